"""Torch-CPU restatement of the segmentation head (JNet on latents and decoder bridges) in float32 or float64, written
from the formulas (include/cae_hip.h "segmentation head"), plus a numpy emulation of the kernels' arithmetic for the
judge test.  It reads a plain state dict with the reference's keys; it is the oracle where the reference is absent.

Stages are named after the layer that produced them ('bottleneck._c1', 'bottleneck._bn1', ...,
'synthesis_track.2._c2', 'fc'): the value right behind that layer, before any ReLU.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
U = 2.0 ** -24
# bound of the statistics behind (a, b), in units of 2^-24 (|a| (|x| + |m|) + |b|) on the effect a x + b (stat_ratio).
# Largest error / bound observed over tests/test_segmenter.py on an MI355X: 6.65 (case E, latents 7 x 15,
# bottleneck._c1: planes of zero-mean outputs, where |m| and |b| are far below sigma); the constant is the next power
# of two above twice that.  The smallest planted defect of the judge test lies at 3205 (tests/test_segmenter_host.py).
C_STAT = 16.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# the golden configurations (tools/gen_segmenter_golden.py): name -> (constructor keys, latent size, batch)
GOLDEN_CONFIGS = {
    'a': (dict(channels_bn=48, channels_net=40, seg_channels_net=8, seg_channels_bn=72, compression_level=3, num_classes=3,
               concat_bridges=True, batch_norm=True), (3, 5), 2),
    'nobn': (dict(channels_bn=12, channels_net=10, seg_channels_net=5, seg_channels_bn=20, compression_level=2,
                  num_classes=1, concat_bridges=True, batch_norm=False), (2, 3), 2),
    'noconcat': (dict(channels_bn=12, channels_net=10, seg_channels_net=6, seg_channels_bn=20, compression_level=2,
                      num_classes=5, concat_bridges=False, batch_norm=True), (3, 2), 2),
}


def load_golden(name):
    """-> (config, state dict, y_q, bridges, logits, stages) of tests/golden/seg_<name>*.npz as float32 tensors"""
    cfg = GOLDEN_CONFIGS[name][0]
    main = np.load(os.path.join(GOLDEN, f'seg_{name}.npz'))
    sd = {k[3:]: torch.from_numpy(main[k]) for k in main.files if k.startswith('sd/')}
    inp = np.load(os.path.join(GOLDEN, f'seg_{name}_inputs.npz'))
    brg = [torch.from_numpy(inp[f'bridge/{i}']) for i in range(sum(k.startswith('bridge/') for k in inp.files))]
    stages, k = {}, 0
    while os.path.exists(os.path.join(GOLDEN, f'seg_{name}_stages{k}.npz')):
        part = np.load(os.path.join(GOLDEN, f'seg_{name}_stages{k}.npz'))
        stages.update({key: torch.from_numpy(part[key]) for key in part.files})
        k += 1
    return cfg, sd, torch.from_numpy(inp['y_q']), brg, torch.from_numpy(main['logits']), stages


def group_norm(x, gamma, beta):
    """GroupNorm with one group per channel: per (sample, channel) mean and biased variance of the plane"""
    m = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - m) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def jnet(sd, cfg, y_q, bridges, dtype=torch.float64):
    """-> (logits, stages) of the head with state dict `sd` (reference keys) in `dtype` on the CPU"""
    sd = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    L, bn, concat = cfg['compression_level'], cfg.get('batch_norm', True), cfg.get('concat_bridges', False)
    stages = {}

    def keep(name, v):
        stages[name] = v
        return v

    def norm_relu(v, prefix):
        if bn:
            v = keep(prefix, group_norm(v, sd[prefix + '.weight'], sd[prefix + '.bias']))
        return torch.relu(v)

    def conv(v, name, pad):
        return keep(name, F.conv2d(v, sd[name + '.weight'], None, padding=pad))

    def up(v, name):
        return keep(name, F.conv_transpose2d(v, sd[name + '.weight'], sd[name + '.bias'], stride=2))

    fx = y_q.detach().cpu().to(dtype)
    fx = norm_relu(conv(fx, 'bottleneck._c1', 0), 'bottleneck._bn1')
    fx = norm_relu(conv(fx, 'bottleneck._c2', 1), 'bottleneck._bn2')
    fx = up(fx, 'bottleneck._up_sample')
    for i in range(L):
        if concat:
            p = f'bridges_projection.{i}'
            b = norm_relu(bridges[i].detach().cpu().to(dtype), p + '._bn1')
            b = norm_relu(conv(b, p + '._c2', 1), p + '._bn2')
            fx = torch.cat((b, fx), dim=1)
        s = f'synthesis_track.{i}'
        fx = norm_relu(conv(fx, s + '._c1', 1), s + '._bn1')
        fx = norm_relu(conv(fx, s + '._c2', 1), s + '._bn2')
        if i + 1 < L:
            fx = up(fx, s + '._up_sample')
    logits = keep('fc', F.conv2d(fx, sd['fc.weight'], sd['fc.bias']))
    return logits, stages


def e2e_bound(f32_logits, f64_logits):
    """the end-to-end requirement: max|got - f64| <= 4 max|f32 restatement - f64| + 1e-6 max|f64|"""
    return 4.0 * float((f32_logits.double() - f64_logits).abs().max()) + 1e-6 * float(f64_logits.abs().max())


# ---------------------------------------------------------------------------------------------------------------
# statistics: what (a, b) must do, and its bound
def stat_ratio(a, b, x, gamma, beta):
    """(a, b) (n, c) judged by its effect xhat = a x + b against float64 statistics of the plane x (n, c, h, w):
    -> max over elements of |xhat - ref| / (2^-24 (|a| (|x| + |m|) + |b|)); the test asserts it <= C_STAT"""
    x = x.detach().cpu().double()
    a, b = a.detach().cpu().double()[:, :, None, None], b.detach().cpu().double()[:, :, None, None]
    m = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    if gamma is None:
        ref = x
    else:
        g, be = gamma.detach().cpu().double().view(1, -1, 1, 1), beta.detach().cpu().double().view(1, -1, 1, 1)
        ref = (x - m) / torch.sqrt(var + EPS) * g + be
    if not (bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())):
        return float('inf')
    bound = U * (a.abs() * (x.abs() + m.abs()) + b.abs())
    return float(((a * x + b - ref).abs() / bound.clamp_min(1e-300)).max())


def staged(x, a, b):
    """v = max(fmaf(a, x, b), 0) in fp32 as the kernels stage it (x (n, c, h, w) fp32; a, b (n, c) fp32): the product
    a x is exact in float64 and the sum rounds once more to fp32, which reproduces the fused operation except in rare
    double-rounding ties"""
    x = x.detach().cpu().float().double()
    t = (a.detach().cpu().float().double()[:, :, None, None] * x + b.detach().cpu().float().double()[:, :, None, None]).float()
    return torch.clamp_min(t, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# numpy emulation of the kernels' arithmetic (judge test): tile partials, Chan merge, (a, b), staging, f16x3 products
def _f32(v):
    return np.asarray(v, dtype=np.float32)


def emu_partial(vals):
    """Welford partial of a tile's valid pixels as the epilogue forms it: the sum in double, the mean rounded to fp32,
    the squared deviations from it in fp32"""
    vals = _f32(vals).ravel()
    if vals.size == 0:
        return 0.0, 0.0, 0.0
    mean = _f32(np.sum(vals.astype(np.float64)) / vals.size)
    return float(vals.size), float(mean), float(np.sum((vals - mean) ** 2, dtype=np.float32))


def emu_merge(p, q):
    """Chan's merge in double; the partials it reads were stored as fp32"""
    (n, mean, m2), (nb, mb, m2b) = p, q
    if nb == 0:
        return p
    if n == 0:
        return q
    nn, d = n + nb, mb - mean
    return nn, mean + d * (nb / nn), m2 + m2b + d * d * (n * nb / nn)


def emu_ab(plane, gamma, beta, tile=(8, 16), defect=None):
    """(a, b) of one (sample, channel) plane (h, w) fp32 through tile partials in tile order"""
    plane = _f32(plane)
    h, w = plane.shape
    ty, tx = tile
    if defect == 'naive_variance':  # E[x^2] - m^2 in fp32
        m = np.mean(plane, dtype=np.float32)
        var = np.maximum(_f32(np.mean(plane * plane, dtype=np.float32) - m * m), _f32(0))  # (clamped, as such code does)
        n, mean, m2 = _f32(plane.size), m, _f32(var * plane.size)
    else:
        acc = (0.0, 0.0, 0.0)
        for y0 in range(0, h, ty):
            for x0 in range(0, w, tx):
                t = plane[y0:y0 + ty, x0:x0 + tx]
                if defect == 'padding_pixels':  # a ragged tile's padding pixels (zeros) counted
                    full = np.zeros(tile, np.float32)
                    full[:t.shape[0], :t.shape[1]] = t
                    t = full
                acc = emu_merge(acc, emu_partial(t))
        n, mean, m2 = acc
    n, mean, m2 = float(n), _f32(mean), float(m2)
    var = _f32(m2 / (n - 1 if defect == 'unbiased' and n > 1 else n))
    rstd = _f32(1.0) / np.sqrt(_f32(var + (0.0 if defect == 'no_eps' else EPS)), dtype=np.float32)
    a = _f32(gamma * rstd)
    return a, _f32(beta - mean * a)


def _split(v):
    hi = _f32(v).astype(np.float16)
    lo = (_f32(v) - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def emu_conv(srcs, w, bias=None, defect=None):
    """stride-1 zero-padded convolution of the concatenated staged sources (each (n, c, h, w) fp32, already v) with
    w (cout, cin, k, k): f16x3 products, wide accumulation (the fp32 accumulation is what C_CONV allows for)"""
    v = np.concatenate([_f32(s) for s in srcs], axis=1)
    if defect == 'b_from_a' and len(srcs) == 2:  # source B's channels read from source A
        v = np.concatenate([_f32(srcs[0]), _f32(srcs[0])[:, :srcs[1].shape[1]]], axis=1)
    vh, vl = (torch.from_numpy(t) for t in _split(v))
    wh, wl = (torch.from_numpy(t) for t in _split(w))
    pad = w.shape[-1] // 2
    out = F.conv2d(vh, wh, padding=pad) + F.conv2d(vh, wl, padding=pad) + F.conv2d(vl, wh, padding=pad)
    if bias is not None:
        out = out + torch.from_numpy(np.asarray(bias, np.float64)).view(1, -1, 1, 1) * (w.shape[-1] ** 2 if defect == 'bias_per_tap' else 1)
    return out.numpy()


def emu_up(v, w, bias, defect=None):
    """2x2 stride-2 transposed convolution as four pointwise matrices with a pixel-shuffle store"""
    n, _, h, wd = v.shape
    cout = w.shape[1]
    out = np.zeros((n, cout, 2 * h, 2 * wd))
    for dy in range(2):
        for dx in range(2):
            wm = np.ascontiguousarray(_f32(w)[:, :, dy, dx].T)[:, :, None, None]  # (cout, cin, 1, 1)
            r = emu_conv([v], wm) + (4 if defect == 'bias_per_tap' else 1) * np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
            py, px = (dx, dy) if defect == 'parity_swapped' else (dy, dx)
            out[:, :, py::2, px::2] = r
    return out
