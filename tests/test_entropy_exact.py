"""Entry points of the entropy model that write every element exactly once, where no test reached.

cae_quantize_export (exported, bound, untested until now), cae_quantize and cae_dequantize against numpy in float32,
bit for bit, at the sizes where the export kernel changes its path: the 16-byte vector kernel with one block (every
thread iterates) and with 32, a total that is no multiple of its step, the scalar kernel for hw % 4 != 0 and for a
destination that is not 16-byte aligned; 1, 24 and 192 channels with medians away from zero; ties and the clamp of
round_sym; and nothing beyond the last element changes.

likelihood_kernel / bits_reduce_kernel against the same density network in float64 on the CPU where
test_gpu_parity.test_likelihood_matches_oracle does not reach: more than one 256-thread pass (hw 255 .. 1000), hidden
widths 6 to 8 and the zero-embedding of narrow layers into the built width, 1, 20 and 320 channels (320: the channel
reduction loops), n = 3.  Tolerances are that test's: y_hat exact, likelihood rtol 1e-4 with the absolute floor of each
form, bits within 1e-5 of -sum log2 of the kernel's own likelihoods.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
LIMIT = 2.0 ** 30  # round_sym clamps to +-2^30 before the conversion; NaN takes the lower clamp


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return cae


def _bottleneck(cae, channels):
    """medians away from zero, on multiples of 1/8: median + tie is exact in float32, so a planted tie is a tie"""
    torch.manual_seed(channels)
    eb = cae.EntropyBottleneck(channels).eval()
    with torch.no_grad():
        shift = torch.round(torch.linspace(-3.3, 2.7, channels) * 8) / 8
        eb.quantiles[:, 0, 1] += torch.where(shift == 0, torch.full_like(shift, 0.125), shift)
    eb.update(force=True)
    med = eb.quantiles[:, 0, 1].detach().numpy().astype(np.float32)
    assert np.all(med != 0.0)
    return eb.cuda(), med


def _latents(n, channels, hw, med, seed):
    y = (np.random.default_rng(seed).standard_normal((n, channels, hw)) * 6).astype(np.float32)
    flat = y.reshape(-1)
    special = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, LIMIT, -LIMIT, LIMIT + 128, -LIMIT - 128, 2.0 ** 31, -2.0 ** 31, 3.0e9,
               -3.0e9, 1.0e20, -1.0e20, np.inf, -np.inf, np.nan]
    at = np.linspace(0, flat.size - 1, len(special)).astype(np.int64)  # first and last element included
    c = (at // hw) % channels
    flat[at] = (np.array(special, dtype=np.float32) + med[c]).astype(np.float32)
    return y


def _symbols(y, med):
    d = (y - med[None, :, None]).astype(np.float32)
    d = np.where(np.isnan(d), np.float32(-LIMIT), np.clip(d, np.float32(-LIMIT), np.float32(LIMIT)))
    return np.rint(d).astype(np.int32)


# (channels, n, hw, max_blocks, destination offset in int32 elements): which kernel, and why the size
EXPORT = [
    (24, 2, 400, 1, 0),      # vector kernel, one block: every thread iterates; 4800 float4 = one step of 4096 and a part
    (192, 3, 1000, 32, 0),   # vector kernel, 32 blocks, 144000 float4 = one step of 131072 and a part
    (192, 3, 100, 32, 0),    # vector kernel, 15 blocks, less than one step
    (1, 3, 8, 32, 0),        # vector kernel, 6 float4 in all
    (1, 2, 4096, 1, 0),
    (24, 2, 35, 32, 0),      # hw % 4 != 0: scalar kernel
    (24, 2, 35, 1, 0),       # ... one block: every thread iterates
    (192, 3, 255, 32, 0),
    (1, 3, 1, 32, 0),
    (1, 1, 1001, 1, 0),
    (24, 2, 400, 32, 1),     # destination 4 bytes off 16-byte alignment: scalar kernel although hw % 4 == 0
    (24, 2, 400, 1, 3),
]


@pytest.mark.parametrize('channels,n,hw,max_blocks,offset', EXPORT)
def test_quantize_export_writes_every_symbol_once_and_nothing_else(cae, poisoned_alloc, channels, n, hw, max_blocks,
                                                                   offset):
    eb, med = _bottleneck(cae, channels)
    y = _latents(n, channels, hw, med, seed=hw)
    want = _symbols(y, med)
    assert y.size < 19 or (want.min() == -2 ** 30 and want.max() == 2 ** 30)  # the clamp is in play
    buf = torch.full((y.size + 64,), SENTINEL, dtype=torch.int32).pin_memory()
    start = 32 + offset  # (pinned memory is page-aligned: element 32 is 16-byte aligned)
    out = buf[start:start + y.size]
    assert out.data_ptr() % 16 == 4 * offset
    eb.quantize_export(torch.from_numpy(y).cuda().view(n, channels, hw), out, max_blocks=max_blocks)
    torch.cuda.synchronize()
    got = buf.numpy()
    assert np.array_equal(got[start:start + y.size].reshape(want.shape), want)
    assert np.all(got[:start] == SENTINEL) and np.all(got[start + y.size:] == SENTINEL)
    poisoned_alloc.check()


@pytest.mark.parametrize('channels,n,hw', sorted({c[:3] for c in EXPORT}))
def test_quantize_and_dequantize_are_exact(cae, poisoned_alloc, channels, n, hw):
    """cae_quantize / cae_dequantize at the shapes of the export test, outputs poisoned and fenced"""
    eb, med = _bottleneck(cae, channels)
    y = _latents(n, channels, hw, med, seed=hw)
    want = _symbols(y, med)
    sym = eb.quantize_symbols(torch.from_numpy(y).cuda())
    assert sym.dtype == torch.int32 and np.array_equal(sym.cpu().numpy(), want)
    back = eb.dequantize_symbols(sym)
    assert np.array_equal(back.cpu().numpy(), want.astype(np.float32) + med[None, :, None])
    poisoned_alloc.check()


# ------------------------------------------------------------------------------------------------- likelihood
def _density64(eb, v):
    """the cumulative-logit network of `eb` in float64; v (C, 1, M)"""
    k = len(eb.filters)
    p = {n: t.detach().double().cpu() for n, t in eb.named_parameters()}
    for i in range(k + 1):
        v = torch.matmul(F.softplus(p[f'_matrix{i}']), v) + p[f'_bias{i}']
        if i < k:
            v = v + torch.tanh(p[f'_factor{i}']) * torch.tanh(v)
    return v


def _reference(eb, y):
    """y (n, C, hw) float32 -> (y_hat in float32 as the kernel forms it, likelihood in float64, bounded below)"""
    med = eb.quantiles[:, 0, 1].detach().float().cpu().numpy()[None, :, None]
    y_hat = (np.rint((y - med).astype(np.float32)) + med).astype(np.float32)
    v = torch.from_numpy(y_hat).double().permute(1, 0, 2).reshape(y.shape[1], 1, -1)
    lo, up = _density64(eb, v - 0.5), _density64(eb, v + 0.5)
    s = -torch.sign(lo + up)  # (the two forms are one function in exact arithmetic; this one does not cancel)
    p = torch.abs(torch.sigmoid(s * up) - torch.sigmoid(s * lo))
    p = torch.clamp(p, min=float(eb.likelihood_lower_bound.bound))
    return y_hat, p.reshape(y.shape[1], y.shape[0], -1).permute(1, 0, 2).numpy()


def _density_model(cae, channels, filters, form):
    torch.manual_seed(5)
    eb = cae.EntropyBottleneck(channels, filters=filters, likelihood_form=form).eval()
    with torch.no_grad():  # non-trivial factors and matrices (init has factor = 0)
        for n, p in eb.named_parameters():
            if n.startswith('_factor'):
                p.uniform_(-1.0, 1.0)
            elif n.startswith('_matrix'):
                p.add_(torch.randn_like(p) * 0.3)
    eb.fit_quantiles()
    eb.update(force=True)
    return eb


def _density_latents(n, channels, hw):
    """inside the support of the fitted tables, and every 7th value far out in the tails, down to the likelihood bound"""
    y = np.random.default_rng(hw + channels).standard_normal((n, channels, hw)) * 6.0
    y.reshape(-1)[::7] *= 40.0
    return y.astype(np.float32)


# (filters, channels, hw)
LIKELIHOOD = [((6,), 20, 257), ((7, 7), 20, 257), ((8, 8, 8), 20, 257), ((2, 8, 3), 20, 257),
              ((8, 8, 8), 20, 1), ((8, 8, 8), 20, 255), ((8, 8, 8), 20, 256), ((8, 8, 8), 20, 1000),
              ((7, 7), 1, 1000), ((7, 7), 320, 257), ((2, 8, 3), 320, 1), ((6,), 1, 1)]
ATOL = {'plain': 2e-7, 'sign_trick': 1e-12}  # (test_likelihood_matches_oracle: plain cancels near sigmoid = 1)


@pytest.mark.parametrize('form', ['plain', 'sign_trick'])
@pytest.mark.parametrize('filters,channels,hw', LIKELIHOOD)
def test_likelihood_against_float64(cae, poisoned_alloc, filters, channels, hw, form):
    n = 3
    eb = _density_model(cae, channels, filters, form)
    y = _density_latents(n, channels, hw)
    y_ref, p_ref = _reference(eb, y)
    eb = eb.cuda()
    y_dev = torch.from_numpy(y).cuda()
    with torch.no_grad():
        y_hat, p = eb(y_dev)
        bits = eb.rate_bits(y_dev)
    poisoned_alloc.check()
    assert np.array_equal(y_hat.cpu().numpy(), y_ref)
    p = p.cpu().numpy()
    err = np.abs(p - p_ref) - ATOL[form]
    print(f'likelihood {filters} C={channels} hw={hw} {form}: max (|err| - atol) / p = {float((err / p_ref).max()):.3e}')
    np.testing.assert_allclose(p, p_ref, rtol=1e-4, atol=ATOL[form])
    assert float(p.min()) >= 1e-9 * (1 - 1e-6)
    assert bits.shape == (n,) and bits.dtype == torch.float64
    np.testing.assert_allclose(bits.cpu().numpy(), -np.log2(p.astype(np.float64)).sum(axis=(1, 2)), rtol=1e-5)
