"""Case generator of the training sweep (fuzz_train.py), importable: `draw_case(rng)` consumes the draws of one case from
np.random.default_rng(seed) in the sweep's order, so `case(seed, k)` rebuilds case k of a sweep; `build(case)` makes its
models and inputs (torch's generator seeded from the case, as the sweep does).  Whether the decoder carries multiscale colour
layers is drawn from a second generator (np.random.default_rng([seed, 1])), so the cases of the earlier sweeps keep their
numbers and everything else they drew."""
import numpy as np
import torch


def draw_case(rng, rng_ms):
    act = rng.choice([None, 'GDN', 'LeakyReLU', 'ReLU'])
    act = None if act is None else str(act)
    groups = bool(rng.integers(0, 4) == 0)
    L = int(rng.integers(1, 4))
    if groups:  # depthwise layers need output channels divisible by the input channels
        c = int(rng.choice([4, 8]))
        enc_kw = dict(channels_org=c, channels_net=2 * c, channels_bn=4 * c)
        dec_kw = dict(channels_org=c, channels_net=c, channels_bn=c)
    else:
        enc_kw = dec_kw = dict(channels_org=int(rng.choice([1, 3])), channels_net=int(rng.choice([8, 32, 40, 64])),
                               channels_bn=int(rng.choice([16, 48, 72])))
    kw = dict(compression_level=L, kernel_size=int(rng.choice([3, 5])), bias=bool(rng.integers(0, 2)), groups=groups,
              batch_norm=bool(rng.integers(0, 3) == 0), use_residual=bool(rng.integers(0, 2)), act_layer_type=act)
    n = int(rng.integers(2, 5))
    h, w = int(rng.integers(2 ** L + 3, 49)), int(rng.integers(2 ** L + 3, 65))
    lh, lw = int(rng.integers(2, 7)), int(rng.integers(2, 9))
    torch_seed = int(rng.integers(0, 1 << 30))
    multiscale = bool(rng_ms.integers(0, 2)) and L > 1
    return dict(kw=kw, enc_kw=enc_kw, dec_kw=dec_kw, shape=(n, h, w), latents=(lh, lw), torch_seed=torch_seed,
                multiscale=multiscale)


def generators(seed):
    return np.random.default_rng(seed), np.random.default_rng([seed, 1])


def case(seed, k):
    """case k of the sweep with this seed"""
    rngs = generators(seed)
    for _ in range(k):
        draw_case(*rngs)
    return draw_case(*rngs)


def describe(k, c):
    return f'case {k}: {c["kw"]} enc {c["enc_kw"]} {c["shape"]} latents {c["latents"]}' + (' multiscale' if c['multiscale'] else '')


def build(c, cae, device='cuda'):
    """-> (encoder, decoder, analysis input, synthesis input): modules in train mode, batch-norm affine parameters and GDN
    gammas moved off their initial values, the draws of torch's generator in the sweep's order"""
    torch.manual_seed(c['torch_seed'])
    enc = cae.Analyzer(**c['enc_kw'], **c['kw']).to(device).train()
    state = torch.get_rng_state()
    dec = cae.Synthesizer(**c['dec_kw'], **c['kw'], multiscale_analysis=c['multiscale']).to(device).train()
    if c['multiscale']:  # (the generator then stands where a plain decoder leaves it: the other draws are the earlier sweeps')
        torch.set_rng_state(state)
        cae.Synthesizer(**c['dec_kw'], **c['kw'])
    with torch.no_grad():
        for mod in list(enc.modules()) + list(dec.modules()):
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.2, 0.2)
            if isinstance(mod, cae.GDN):
                mod.gamma.add_(0.05 * torch.rand_like(mod.gamma))
    n, h, w = c['shape']
    x = torch.rand(n, c['enc_kw']['channels_org'], h, w)
    yq = 2.0 * torch.randn(n, c['dec_kw']['channels_bn'], *c['latents'])
    return enc, dec, x, yq
