"""GDN / IGDN (both forms), the entropy-bottleneck density, the NonNegativeParametrizer and the clip + Adam step: each
training entry point called directly through the C ABI and compared element by element with a float64 computation of
the same operation on the same fp32 operands.  Bounds are first-order error bounds (tests/train_bounds.py): an fp32 sum
contributes C * 2^-24 * sum|terms|, an elementary function a stated ulp constant, an input the error it already carries.

Every output buffer is pre-filled with NaN (an element the kernel never writes fails), padded channels must come out
exactly 0, and no output may be NaN or Inf.

The *_judge_rejects_* tests (no GPU) show that the GDN and density bounds pass a float32 emulation of the kernels'
arithmetic under several summation orders and fail each planted defect.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import train_bounds as TB

U = TB.U
CAE_ERR_UNSUPPORTED = -4


def _L():
    from cnn_autoencoder_amd import _lib
    return _lib.lib()


def _check(rc):
    from cnn_autoencoder_amd import _lib
    _lib.check(rc)


def _pad32(c):
    return (c + 31) // 32 * 32


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device='cuda')


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


# ================================================================================================================ GDN
def gdn_operands(c, n, h, w, pad, seed):
    """fp32 operands: z spanning 2^-10 .. 2^6 with whole pixels of zeros; Gamma not symmetric, off-diagonal entries as
    large as the diagonal, a fifth of them at the reparametrisation floor 0; beta at its effective floor 1e-6 on every
    other channel, about 1 on the rest; the extended-domain gradient g_ext [n][h + 2 pad][w + 2 pad][c]"""
    gen = torch.Generator().manual_seed(seed)
    P = n * h * w
    z = torch.exp2(torch.rand(P, c, generator=gen) * 16 - 10) * (torch.randint(0, 2, (P, c), generator=gen) * 2 - 1)
    z[::7] = 0.0
    gamma = torch.rand(c, c, generator=gen) * (torch.rand(c, c, generator=gen) > 0.2)
    beta = torch.where(torch.arange(c) % 2 == 0, torch.full((c,), 1e-6), 0.5 + torch.rand(c, generator=gen))
    gext = torch.randn(n, h + 2 * pad, w + 2 * pad, c, generator=gen)
    return z.float(), beta.float(), gamma.float(), gext.float()


def _padded(z, beta, gamma, gext, cp):
    """the kernels' padding: z, g_ext 0, beta 1, Gamma 0"""
    c = z.shape[1]
    zp = torch.zeros(z.shape[0], cp)
    zp[:, :c] = z
    bp = torch.ones(cp)
    bp[:c] = beta
    gp = torch.zeros(cp, cp)
    gp[:c, :c] = gamma
    ep = torch.zeros(*gext.shape[:-1], cp)
    ep[..., :c] = gext
    return zp.cuda(), bp.cuda(), gp.cuda(), ep.cuda()


def run_gdn(form, z, beta, gamma, gext, shape, pad, inverse):
    """-> dict of the outputs (padded, on the GPU) of the three-kernel form or the fused pair"""
    L = _L()
    n, h, w = shape
    c = z.shape[1]
    cp = _pad32(c)
    P = n * h * w
    zd, bd, gd, ed = _padded(z, beta, gamma, gext, cp)
    o = {}
    if form == 'three':
        o['y32'], o['y16'] = _nan((P, cp)), _nan((P, cp), torch.bfloat16)
        _check(L.cae_t_gdn_forward(zd.data_ptr(), P, cp, bd.data_ptr(), gd.data_ptr(), int(inverse), o['y32'].data_ptr(),
                                   o['y16'].data_ptr(), None))
        gtd = gd.t().contiguous()
        ws1, ws2 = _nan((P, cp)), _nan((P, cp))
        o['gz32'], o['gz16'] = _nan((P, cp)), _nan((P, cp), torch.bfloat16)
        o['ggamma'], o['gbeta'] = _nan((cp, cp)), _nan((cp,))
        _check(L.cae_t_gdn_backward(zd.data_ptr(), ed.data_ptr(), n, h, w, pad, cp, bd.data_ptr(), gd.data_ptr(),
                                    gtd.data_ptr(), int(inverse), ws1.data_ptr(), ws2.data_ptr(), o['gz32'].data_ptr(),
                                    o['gz16'].data_ptr(), o['ggamma'].data_ptr(), o['gbeta'].data_ptr(), None))
    else:
        ne = L.cae_t_gdn_saved_elems(P, cp)
        assert ne >= P * cp
        f = _nan((ne,))
        o['y16'] = _nan((P, cp), torch.bfloat16)
        _check(L.cae_t_gdn_forward_save(zd.data_ptr(), P, cp, bd.data_ptr(), gd.data_ptr(), int(inverse), o['y16'].data_ptr(),
                                        f.data_ptr(), None))
        ge = ed.clone()  # (folded in place)
        o['gz16'] = _nan((P, cp), torch.bfloat16)
        o['ggamma'], o['gbeta'] = _nan((cp, cp)), _nan((cp,))
        _check(L.cae_t_gdn_backward_fused(zd.data_ptr(), f.data_ptr(), ge.data_ptr(), n, h, w, pad, cp, gd.data_ptr(),
                                          int(inverse), o['gz16'].data_ptr(), o['ggamma'].data_ptr(), o['gbeta'].data_ptr(),
                                          None))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


# (n, h, w, pad): 1, 31, 33 pixels; 65 .. 68 (the saved factor's 64-pixel granularity); images of P + 1 and P + 2 rows /
# columns, odd x even; just above 8 192 (fused backward: 256 tiles), 16 384 (fused forward: 512 tiles) and 131 072 pixels
# (three-kernel form: 512 blocks x 256 pixels), each with a ragged last tile
SMALL = [(1, 1, 1, 0), (1, 1, 31, 0), (1, 3, 11, 1), (1, 5, 13, 2), (1, 3, 22, 2), (2, 2, 3, 1), (1, 4, 17, 2)]
LARGE = [(2, 64, 65, 1), (1, 129, 129, 2), (2, 257, 257, 1)]
GDN_CHANNELS = [1, 3, 32, 40, 96, 128, 160, 192]


def _gdn_cases():
    cases = []
    for c in GDN_CHANNELS:
        for form in ('three', 'fused'):
            if form == 'three' or _pad32(c) <= 128:  # (above: test_fused_gdn_refuses_more_than_128_channels)
                for si, s in enumerate(SMALL):
                    cases.append((c, s, form, (si + c) % 2))
    for s in LARGE[:2]:
        for c in (40, 128):
            for form in ('three', 'fused'):
                cases.append((c, s, form, c % 3 % 2))
    cases += [(192, LARGE[2], 'three', 0), (160, LARGE[2], 'three', 1), (128, LARGE[2], 'fused', 1)]
    return cases


WORST = {}


def _judge(got, ref, B, what, key):
    r = TB.judge(got, ref, B, what)
    WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.mark.gpu
@pytest.mark.parametrize('c,shape,form,inverse', _gdn_cases())
def test_gdn_against_float64(cae, c, shape, form, inverse):
    """y (fp32 / bf16), g_z (bf16, and fp32 from the three-kernel form), g_Gamma and g_beta against the float64 GDN / IGDN
    and its backward; padded channels exactly 0"""
    n, h, w, pad = shape
    cp = _pad32(c)
    z, beta, gamma, gext = gdn_operands(c, n, h, w, pad, seed=c * 1000 + h * w + pad)
    o = run_gdn(form, z, beta, gamma, gext, (n, h, w), pad, inverse)
    R = TB.gdn_reference(z, beta, gamma, inverse, gext, (n, h, w), pad)
    tag = f'gdn {form} {"igdn" if inverse else "gdn"} c {c} {(n, h, w)} pad {pad}'
    for k in o:
        assert bool(torch.isfinite(o[k].float()).all()), (tag, k)
    if 'y32' in o:
        _judge(o['y32'][:, :c], R['y'], R['B_y'], tag + ' y32', f'{form} y32')
    _judge(o['y16'][:, :c], R['y'], R['B_y'] + TB.bf16_ulp(R['y']), tag + ' y16', f'{form} y16')
    if 'gz32' in o:
        _judge(o['gz32'][:, :c], R['gz'], R['B_gz'], tag + ' gz32', f'{form} gz32')
    _judge(o['gz16'][:, :c], R['gz'], R['B_gz'] + TB.bf16_ulp(R['gz']), tag + ' gz16', f'{form} gz16')
    _judge(o['ggamma'][:c, :c], R['ggamma'], R['B_ggamma'], tag + ' ggamma', f'{form} ggamma')
    _judge(o['gbeta'][:c], R['gbeta'], R['B_gbeta'], tag + ' gbeta', f'{form} gbeta')
    if cp > c:
        for k in ('y32', 'y16', 'gz32', 'gz16'):
            if k in o:
                assert float(o[k][:, c:].float().abs().max()) == 0.0, (tag, k)
        assert float(o['ggamma'][c:, :].abs().max()) == 0.0 and float(o['ggamma'][:, c:].abs().max()) == 0.0, tag
        assert float(o['gbeta'][c:].abs().max()) == 0.0, tag


@pytest.mark.gpu
@pytest.mark.parametrize('c', [160, 192])
def test_fused_gdn_refuses_more_than_128_channels(cae, c):
    """the fused pair is built for at most 128 channels: CAE_ERR_UNSUPPORTED before any launch, no saved-factor size"""
    L = _L()
    cp, P = _pad32(c), 64
    z, beta, gamma, gext = gdn_operands(c, 1, 8, 8, 1, seed=c)
    zd, bd, gd, ed = _padded(z, beta, gamma, gext, cp)
    assert L.cae_t_gdn_saved_elems(P, cp) == 0
    f, y16 = _nan((P * cp,)), _nan((P, cp), torch.bfloat16)
    assert L.cae_t_gdn_forward_save(zd.data_ptr(), P, cp, bd.data_ptr(), gd.data_ptr(), 0, y16.data_ptr(), f.data_ptr(),
                                    None) == CAE_ERR_UNSUPPORTED
    gz16, gg, gb = _nan((P, cp), torch.bfloat16), _nan((cp, cp)), _nan((cp,))
    assert L.cae_t_gdn_backward_fused(zd.data_ptr(), f.data_ptr(), ed.data_ptr(), 1, 8, 8, 1, cp, gd.data_ptr(), 0,
                                      gz16.data_ptr(), gg.data_ptr(), gb.data_ptr(), None) == CAE_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(y16.float()).all()) and bool(torch.isnan(gz16.float()).all())


GDN_DEFECTS = ['fold_skips_row0', 'clamped_rows_in_ggamma', 'gamma_for_gamma_t', 'drop_cross_term_on_tile_1',
               'last_tile_reads_previous_f']


def test_gdn_judge_rejects_wrong_kernels():
    """The GDN bounds pass a float32 emulation of the fused kernels under several summation orders and fail each planted
    defect (40 channels: two channel tiles, the second ragged; 2 x 37 pixels with pad 1: H = P + 1, three 32-pixel
    tiles, the last one ragged)."""
    shape, pad = (1, 2, 37), 1
    for inverse in (0, 1):
        z, beta, gamma, gext = gdn_operands(40, *shape, pad, seed=5 + inverse)
        R = TB.gdn_reference(z, beta, gamma, inverse, gext, shape, pad)

        def worst(outs):
            y, gz, gg, gb = outs
            return max(TB.ratio(y, R['y'], R['B_y']), TB.ratio(gz, R['gz'], R['B_gz']),
                       TB.ratio(gg, R['ggamma'], R['B_ggamma']), TB.ratio(gb, R['gbeta'], R['B_gbeta']))
        for seed in range(3):
            r = worst(TB.emulate_gdn(z, beta, gamma, inverse, gext, shape, pad, seed))
            TB.report(f'gdn emulation inverse {inverse} order {seed}', r)
            assert r <= 1.0, (inverse, seed, r)
        for mut in GDN_DEFECTS:
            r = worst(TB.emulate_gdn(z, beta, gamma, inverse, gext, shape, pad, 0, mut))
            TB.report(f'gdn defect {mut} inverse {inverse}', r)
            assert r > 1.0, (mut, inverse, r)


# ============================================================================================================ density
BOUND = float(np.float32(1e-9))  # (the kernels clamp at the fp32 value of the likelihood bound)


def density_raw(C, regime, seed):
    """raw parameters (C, NP) fp32: EntropyBottleneck's initial values ('init'), perturbed ('perturbed': one raw matrix
    entry at 21.5, above the softplus threshold), or perturbed with zero biases ('symmetric': odd logits, so v = 0 gives
    lower + upper = 0 and the sign trick's sign(0) = 0)"""
    gen = torch.Generator().manual_seed(seed)
    raw = torch.zeros(C, TB.NP, dtype=torch.float64)
    filters = (1, 3, 3, 3, 3, 1)
    scale = 10.0 ** (1 / 5)
    for i in range(TB.K + 1):
        n = TB.DOUT[i] * TB.DIN[i]
        raw[:, TB.M_OFF[i]:TB.M_OFF[i] + n] = math.log(math.expm1(1 / scale / filters[i + 1]))
        raw[:, TB.B_OFF[i]:TB.B_OFF[i] + TB.DOUT[i]] = torch.rand(C, TB.DOUT[i], generator=gen, dtype=torch.float64) - 0.5
    if regime != 'init':
        raw[:, :TB.NM] += 0.2 * torch.randn(C, TB.NM, generator=gen, dtype=torch.float64)
        raw[:, TB.NM + TB.NB:] = 0.3 * torch.randn(C, TB.NP - TB.NM - TB.NB, generator=gen, dtype=torch.float64)
        raw[0, TB.M_OFF[2] + 4] = 21.5
    if regime == 'symmetric':
        raw[:, TB.NM:TB.NM + TB.NB] = 0.0
    return raw.float()


def _search(raw, target, side, plain):
    """per channel, v on `side` of 0 with p(v) = target (bisection in float64 between 0 and 300 side)"""
    C = raw.shape[0]
    a, b = torch.zeros(C, 1, dtype=torch.float64), torch.full((C, 1), 300.0 * side, dtype=torch.float64)
    for _ in range(60):
        m = 0.5 * (a + b)
        hi = TB.density_p(raw, m, plain) > target
        a, b = torch.where(hi, m, a), torch.where(hi, b, m)
    return a.float()


def density_inputs(raw, E, plain, seed, noise, specials=True):
    """y (C, E) fp32: 4 randn, plus at evenly spaced elements (the first and the last included): the tails +-300 (clamped
    to the bound), elements 1 % either side of the clamp on both sides, the plain form's cancellation region on the right
    (p = 1e-7, 1e-5: sigmoid(u) ~ sigmoid(l) ~ 1), its left mirror, zeros and 0.5; noise U(-1/2, 1/2) or None (0 at the
    special elements)"""
    gen = torch.Generator().manual_seed(seed)
    C = raw.shape[0]
    y = 4 * torch.randn(C, E, generator=gen)
    if not specials:
        return y.float(), (torch.rand(C, E, generator=gen) - 0.5 if noise else None), None
    specials = [torch.full((C, 1), 300.0), torch.full((C, 1), -300.0)]
    for side in (-1, 1):
        for t in (0.99 * BOUND, 1.01 * BOUND, 1e-5):
            specials.append(_search(raw, t, side, plain))
    specials += [_search(raw, 1e-7, 1, plain), torch.zeros(C, 1), torch.zeros(C, 1), torch.full((C, 1), 0.5)]
    pos = torch.unique(torch.linspace(0, E - 1, len(specials)).round().long())
    for i, p in enumerate(pos.tolist()):
        y[:, p:p + 1] = specials[i]
    nz = None
    if noise:
        nz = torch.rand(C, E, generator=gen) - 0.5
        nz[:, pos] = 0.0
    return y.float(), nz, pos


def _to_nchw(x, N):
    """(C, N HW) -> (N, C, HW) contiguous"""
    C = x.shape[0]
    return x.reshape(C, N, -1).permute(1, 0, 2).contiguous()


def _from_nchw(x):
    N, C = x.shape[:2]
    return x.permute(1, 0, 2).reshape(C, -1)


def run_density(raw, y, noise, g_lik, g_out, N, plain):
    L = _L()
    C, E = y.shape
    HW = E // N
    yd = _to_nchw(y, N).cuda()
    nd = None if noise is None else _to_nchw(noise, N).cuda()
    rd = raw.cuda().contiguous()
    out, lik = _nan((N, C, HW)), _nan((N, C, HW))
    _check(L.cae_t_density_forward(yd.data_ptr(), None if nd is None else nd.data_ptr(), rd.data_ptr(), N, C, HW, int(plain),
                                   BOUND, out.data_ptr(), lik.data_ptr(), None))
    gld = _to_nchw(g_lik, N).cuda()
    god = None if g_out is None else _to_nchw(g_out, N).cuda()
    gy, graw = _nan((N, C, HW)), _nan((C, TB.NP))
    _check(L.cae_t_density_backward(out.data_ptr(), gld.data_ptr(), None if god is None else god.data_ptr(), rd.data_ptr(),
                                    N, C, HW, int(plain), BOUND, gy.data_ptr(), graw.data_ptr(), None))
    torch.cuda.synchronize()
    return _from_nchw(out.cpu()), _from_nchw(lik.cpu()), _from_nchw(gy.cpu()), graw.cpu()


# elements per channel as (N, HW): 1, 255, 2 048 and 2 049 (one block, then two), 65 536 and 65 537 (32 blocks, then the
# element loop); the canonical batch 128 x 16^2 at 192 channels
DENSITY_SIZES = [(1, 1), (3, 85), (2, 1024), (3, 683), (16, 4096), (1, 65537)]
REGIMES = ['init', 'perturbed', 'symmetric']


def _density_cases():
    cases, i = [], 0
    for C in (1, 3):
        for N, HW in DENSITY_SIZES:
            for plain in (1, 0):
                cases.append((C, N, HW, plain, REGIMES[i % 3], i % 2 == 0, (i // 2) % 2 == 0, 'rate' if i % 4 in (0, 3) else 'random'))
                i += 1
    cases += [(192, 128, 256, 1, 'perturbed', True, True, 'random'), (192, 128, 256, 0, 'symmetric', True, False, 'rate')]
    return cases


def density_g(y, noise, glik_kind, with_gout, N, plain, raw, seed):
    C, E = y.shape
    gen = torch.Generator().manual_seed(seed + 1)
    v = y if noise is None else (y + noise)
    if glik_kind == 'rate':  # d/dlik of -sum log2(lik) / (B H W): negative, passes the LowerBound everywhere
        lik = TB.density_p(raw, v, plain).clamp_min(BOUND).float().double()
        g_lik = (-1.0 / (lik * math.log(2) * N * E / N)).float()
    else:
        g_lik = torch.randn(C, E, generator=gen)
    g_out = torch.randn(C, E, generator=gen) if with_gout else None
    return v, g_lik, g_out


def judge_density(raw, v, g_lik, g_out, plain, lik, gy, graw, tag, key=None, check_autograd=False):
    R = TB.density_reference(raw, v, g_lik, g_out, plain, BOUND)
    if check_autograd:  # the hand-written float64 backward is the oracle's graph under autograd
        gy_a, graw_a = TB.density_autograd(raw, v, g_lik, g_out, plain, BOUND)
        assert torch.allclose(R['g_y'], gy_a, rtol=1e-9, atol=1e-12 * float(gy_a.abs().max())), tag
        assert torch.allclose(R['g_raw'], graw_a, rtol=1e-9, atol=1e-12 * float(graw_a.abs().max())), tag
    rs = [TB.ratio(lik, R['lik'], R['B_lik']), TB.ratio(gy, R['g_y'], R['B_gy']), TB.ratio(graw, R['g_raw'], R['B_graw'])]
    if key is not None:
        for name, r in zip(('lik', 'g_y', 'g_raw'), rs):
            TB.report(f'{tag} {name}', r)
            WORST[f'density {name}'] = max(WORST.get(f'density {name}', 0.0), r)
            assert r <= 1.0, (tag, name, r)
    return max(rs)


@pytest.mark.gpu
@pytest.mark.parametrize('C,N,HW,plain,regime,noise,with_gout,glik', _density_cases())
def test_density_against_float64(cae, C, N, HW, plain, regime, noise, with_gout, glik):
    """cae_t_density_forward / backward: out == y + noise exactly, lik, g_y and the gradient of every raw parameter
    within the propagated float64 bound (192 channels: every output is finite, 25 channels are judged element by
    element)"""
    seed = C * 100 + HW + plain
    raw = density_raw(C, regime, seed)
    E = N * HW
    y, nz, _ = density_inputs(raw, E, plain, seed, noise)
    v, g_lik, g_out = density_g(y, nz, glik, with_gout, N, plain, raw, seed)
    out, lik, gy, graw = run_density(raw, y, nz, g_lik, g_out, N, plain)
    tag = f'density {"plain" if plain else "sign"} C {C} {N}x{HW} {regime} noise {noise} g_out {with_gout} g_lik {glik}'
    assert torch.equal(out, v), tag + ': out is not y + noise rounded once'
    for t in (lik, gy, graw):
        assert bool(torch.isfinite(t).all()), tag
    assert float(lik.min()) >= BOUND * (1 - 1e-7), tag
    sel = torch.arange(C)
    if C > 8:  # (the float64 bound costs ~0.4 s per channel at 32 768 elements: every 8th channel and the last one)
        sel = torch.cat([torch.arange(0, C, 8), torch.tensor([C - 1])])
    judge_density(raw[sel], v[sel], g_lik[sel], None if g_out is None else g_out[sel], plain, lik[sel].double(),
                  gy[sel].double(), graw[sel].double(), tag, key=True, check_autograd=C * E <= 300000)


DENSITY_DEFECTS = ['softplus_threshold_4', 'lowerbound_inverted', 'drop_last_loop_round', 'one_minus_t']


def test_density_judge_rejects_wrong_kernels():
    """The density bounds pass a float32 emulation of the kernels under several summation orders, for both forms, and
    fail each planted defect (3 channels x 100 000 elements: 32 blocks, 13 rounds of the element loop).

    The softplus threshold is planted at 4, not 15: above 15, log1p(exp(x)) - x < e^-15 = 5.1 u relative and
    1 - sigmoid(x) < 5.1 u, below the rounding of the values themselves; the propagated bound of a parameter gradient is
    ~1e-3 relative here (five layers, cancelling sums), so the threshold defect is resolved from e^-x ~ 1e-2 on."""
    E = 100000
    for plain in (1, 0):
        raw = density_raw(3, 'perturbed', 7 + plain)
        raw[1, TB.M_OFF[1] + 2] = 4.5  # (between 4 and 20)
        worst_defect = {m: 0.0 for m in DENSITY_DEFECTS}
        # (random signs: parameter gradients cancel; the rate loss's do not, but its 1 / lik weights the tails, whose
        # bounds are wide -- without the special elements the rate loss gives the tightest parameter-gradient bounds)
        for glik, special in (('rate', True), ('random', True), ('rate', False)):
            y, nz, _ = density_inputs(raw, E, plain, 3, True, special)
            v, g_lik, g_out = density_g(y, nz, glik, True, 1, plain, raw, 3)
            R = TB.density_reference(raw, v, g_lik, g_out, plain, BOUND)
            gy_a, graw_a = TB.density_autograd(raw, v, g_lik, g_out, plain, BOUND)
            assert torch.allclose(R['g_y'], gy_a, rtol=1e-9, atol=1e-12 * float(gy_a.abs().max()))
            assert torch.allclose(R['g_raw'], graw_a, rtol=1e-9, atol=1e-12 * float(graw_a.abs().max()))

            def worst(outs):
                lik, gy, graw = outs
                return max(TB.ratio(lik, R['lik'], R['B_lik']), TB.ratio(gy, R['g_y'], R['B_gy']),
                           TB.ratio(graw, R['g_raw'], R['B_graw']))
            for seed in range(3):
                r = worst(TB.emulate_density(raw, v, g_lik, g_out, plain, BOUND, seed))
                TB.report(f'density emulation {"plain" if plain else "sign"} g_lik {glik} order {seed}', r)
                assert r <= 1.0, (plain, glik, seed, r)
            for mut in DENSITY_DEFECTS:
                worst_defect[mut] = max(worst_defect[mut], worst(TB.emulate_density(raw, v, g_lik, g_out, plain, BOUND, 0, mut)))
        for mut, r in worst_defect.items():
            TB.report(f'density defect {mut} {"plain" if plain else "sign"}', r)
            assert r > 1.0, (mut, plain, r)


# ============================================================================================================ reparam
@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 257, 600001])
def test_reparam_against_float64(cae, n):
    """cae_t_reparam_forward within the two fp32 roundings of max(x, bound)^2 - pedestal; cae_t_reparam_backward exactly
    the fp32 rounding of g 2 max(x, bound) where x >= bound or that product is negative, else 0 (the product of two fp32
    values is exact in float64, so the mask and the value are checked exactly).  n > 524 288: the grid-stride loop."""
    from oracle import cae_oracle as O
    gen = torch.Generator().manual_seed(n)
    ped = float(np.float32(O.PEDESTAL))
    for minimum in (0.0, 1e-6):
        bound = float(np.float32((minimum + O.PEDESTAL) ** 0.5))
        x = torch.rand(n, generator=gen) * 0.2
        special = torch.tensor([bound, bound * (1 - 2 ** -20), bound * 0.5, -1.0, 0.0, -bound])
        x[:min(n, 6)] = special[:min(n, 6)]
        if n > 6:
            x[-1] = bound
        g = torch.randn(n, generator=gen)
        xd, gd = x.cuda(), g.cuda()
        out, gx = _nan((n,)), _nan((n,))
        _check(_L().cae_t_reparam_forward(xd.data_ptr(), n, bound, ped, out.data_ptr(), None))
        _check(_L().cae_t_reparam_backward(xd.data_ptr(), gd.data_ptr(), n, bound, gx.data_ptr(), None))
        torch.cuda.synchronize()
        c = x.double().clamp_min(bound)
        ref = c * c - ped
        B = U * (c * c + ref.abs()) + TB.TINY
        TB.judge(out.cpu(), ref, B, f'reparam forward n {n} minimum {minimum}')
        gi = g.double() * 2 * c
        want = torch.where((x.double() >= bound) | (gi < 0), gi, torch.zeros_like(gi)).float()
        assert torch.equal(gx.cpu(), want), (n, minimum)


# ========================================================================================================= clip + Adam
SIZES = [1, 2047, 2048, 2049, 3 * 2048 + 5]


def _adam_reference(p, g, m, v, group, cfg):
    """float64 clip_grad_norm_ per group, then torch.optim.Adam (L2 weight decay, bias corrections at the given step)"""
    outs = [None] * len(p)
    for gi, (lr, b1, b2, eps, wd, max_norm, step) in enumerate(cfg):
        idx = [i for i in range(len(p)) if group[i] == gi]
        ps = [p[i].double().clone().requires_grad_(True) for i in idx]
        for q, i in zip(ps, idx):
            q.grad = g[i].double().clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        for q, i in zip(ps, idx):
            opt.state[q] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m[i].double().clone(),
                            'exp_avg_sq': v[i].double().clone()}
        opt.step()
        for q, i in zip(ps, idx):
            outs[i] = (q.detach(), opt.state[q]['exp_avg'], opt.state[q]['exp_avg_sq'])
    return outs


def _adam_bound(p, g, m, v, coef, Ecoef, lr, b1, b2, eps, wd, step):
    """EV replay of the kernel's update of one tensor -> (p, m, v) bounds"""
    A = TB.EVA
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    bc1 = 1 - b1 ** step
    bc2s = math.sqrt(1 - b2 ** step)
    gi = A.mul(g.double(), TB.EV(torch.full_like(g.double(), coef), torch.full_like(g.double(), Ecoef)))
    if wd != 0:
        gi = A.add(gi, A.mul(f32(wd), p.double()))
    mi = A.add(m.double(), A.mul(A.sub(gi, m.double()), A.sub(1.0, f32(b1))))
    vi = A.add(A.mul(f32(b2), v.double()), A.mul(A.mul(A.sub(1.0, f32(b2)), gi), gi))
    step_size = TB.EV(torch.tensor(lr / bc1), torch.tensor(2 * U * lr / bc1))  # (lr / fp32(bc1), rounded)
    den = A.add(A.div(A.sqrt(vi), TB.EV(torch.tensor(bc2s), torch.tensor(U * bc2s))), f32(eps))
    pi = A.sub(p.double(), A.mul(step_size, A.div(mi, den)))
    return pi.e, mi.e, vi.e


@pytest.mark.gpu
def test_clip_adam_against_float64(cae):
    """cae_t_clip_adam with 8 groups and 64 tensors (both CAE_OPTIM_MAX_* limits exactly), tensors of 1, 2 047, 2 048,
    2 049 and 3 x 2 048 + 5 elements (one chunk, a chunk boundary, straddling chunks): param, exp_avg and exp_avg_sq element
    by element against float64 clip_grad_norm_ + torch.optim.Adam.  Groups: max_norm 0 and -1 (no clipping), a clip that
    is active and one that is not; steps 1 and 1 000; weight decay 0 and 1e-2.  The clip coefficient's fp32 sum enters each
    bound explicitly."""
    gen = torch.Generator().manual_seed(0)
    G, NT = 8, 64
    group = [t * G // NT for t in range(NT)]
    p = [torch.randn(SIZES[t % 5], generator=gen) for t in range(NT)]
    g = [torch.randn(SIZES[t % 5], generator=gen) * (0.1 + t % 3) for t in range(NT)]
    norms = [math.sqrt(sum(float((g[t].double() ** 2).sum()) for t in range(NT) if group[t] == gi)) for gi in range(G)]
    cfg = []
    for gi in range(G):
        kind = gi % 4
        max_norm = (0.0, -1.0, 0.25 * norms[gi], 4.0 * norms[gi])[kind]
        step = 1 if gi < 4 else 1000
        cfg.append((float(np.float32(1e-3 * (gi + 1))), float(np.float32(0.9)), float(np.float32(0.999)),
                    float(np.float32(1e-8)), float(np.float32(1e-2 if gi % 2 else 0.0)), float(np.float32(max_norm)), step))
    m = [torch.zeros_like(t) if cfg[group[i]][6] == 1 else 0.01 * torch.randn(t.shape, generator=gen) for i, t in enumerate(p)]
    v = [torch.zeros_like(t) if cfg[group[i]][6] == 1 else 1e-4 * torch.rand(t.shape, generator=gen) for i, t in enumerate(p)]
    pd, gd, md, vd = ([t.cuda() for t in ts] for ts in (p, g, m, v))
    vp = lambda ts: (ctypes.c_void_p * NT)(*[t.data_ptr() for t in ts])  # noqa: E731
    fl = lambda k: (ctypes.c_float * G)(*[c[k] for c in cfg])  # noqa: E731
    chunks = sum((t.numel() + 2047) // 2048 for t in p)
    ws = _nan((chunks,))
    _check(_L().cae_t_clip_adam(NT, vp(pd), vp(gd), vp(md), vp(vd), (ctypes.c_int * NT)(*[t.numel() for t in p]),
                                (ctypes.c_int * NT)(*group), G, fl(0), fl(1), fl(2), fl(3), fl(4), fl(5),
                                (ctypes.c_int * G)(*[c[6] for c in cfg]), ws.data_ptr(), chunks, None))
    torch.cuda.synchronize()
    ref = _adam_reference(p, g, m, v, group, cfg)
    for gi in range(G):
        lr, b1, b2, eps, wd, max_norm, step = cfg[gi]
        if max_norm > 0:
            c = min(max_norm / (norms[gi] + 1e-6), 1.0)
            # norm^2: an fp32 sum of non-negative terms (C_SUM u relative), sqrt, + 1e-6, the division
            Ec = c * (0.5 * TB.C_SUM * U + 2 * U + U + U) if c < 1 else 0.0
            assert (c < 1) == (gi % 4 == 2)
        else:
            c, Ec = 1.0, 0.0
        for t in (i for i in range(NT) if group[i] == gi):
            Bp, Bm, Bv = _adam_bound(p[t], g[t], m[t], v[t], c, Ec, lr, b1, b2, eps, wd, step)
            tag = f'clip_adam group {gi} tensor {t} n {p[t].numel()}'
            TB.judge(pd[t].cpu(), ref[t][0], Bp, tag + ' param')
            TB.judge(md[t].cpu(), ref[t][1], Bm, tag + ' exp_avg')
            TB.judge(vd[t].cpu(), ref[t][2], Bv, tag + ' exp_avg_sq')
