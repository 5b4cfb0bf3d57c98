"""Differentiable torch-CPU restatement of the segmentation head in float32 or float64 (``segmenter_restatement.jnet``
detaches its weights), the losses of head training, and numpy emulations of the backward kernels' arithmetic in their own
order (f16x3 products, segment partials, ordered merge) for the judge tests.  The gradient goldens
(tests/golden/seg_grad_<name>.npz, tools/gen_segmenter_grad_golden.py) come from the reference's own JNet in float64.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import segmenter_restatement as SR

EPS = SR.EPS
U = SR.U


def load_grad_golden(name):
    """-> (target, loss, {parameter key: gradient}) of tests/golden/seg_grad_<name>*.npz (float64)"""
    arrays, k = {}, 0
    path = os.path.join(SR.GOLDEN, f'seg_grad_{name}.npz')
    while os.path.exists(path):
        part = np.load(path)
        arrays.update({key: part[key] for key in part.files})
        k += 1
        path = os.path.join(SR.GOLDEN, f'seg_grad_{name}_{k}.npz')
    grads = {key[5:]: torch.from_numpy(v) for key, v in arrays.items() if key.startswith('grad/')}
    return torch.from_numpy(arrays['target']), float(arrays['loss']), grads


def make_target(name, seed=0):
    """the seeded target of a golden configuration: (n, 1, H, W) float {0, 1} for one class, else (n, H, W) int64"""
    cfg, (lh, lw), n = SR.GOLDEN_CONFIGS[name]
    L, C = cfg['compression_level'], cfg['num_classes']
    gen = torch.Generator().manual_seed(1000 + seed + sum(map(ord, name)))
    shape = (n, lh * 2 ** L, lw * 2 ** L)
    if C == 1:
        return torch.randint(0, 2, (n, 1) + shape[1:], generator=gen).double()
    return torch.randint(0, C, shape, generator=gen)


def head_loss(logits, target):
    """BCEWithLogits (mean) for one class, CrossEntropy (mean) otherwise"""
    if logits.size(1) == 1:
        return F.binary_cross_entropy_with_logits(logits, target.to(logits.dtype))
    return F.cross_entropy(logits, target.long())


def group_norm(x, gamma, beta):
    m = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - m) / torch.sqrt(var + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def jnet_forward(sd, cfg, y_q, bridges):
    """logits of the head with the (differentiable) tensors of `sd`, in their dtype"""
    L, bn, concat = cfg['compression_level'], cfg.get('batch_norm', True), cfg.get('concat_bridges', False)

    def norm_relu(v, prefix):
        return torch.relu(group_norm(v, sd[prefix + '.weight'], sd[prefix + '.bias']) if bn else v)

    def unit(v, p, pad, up):
        v = norm_relu(F.conv2d(v, sd[p + '._c1.weight'], None, padding=pad), p + '._bn1')
        v = norm_relu(F.conv2d(v, sd[p + '._c2.weight'], None, padding=1), p + '._bn2')
        return F.conv_transpose2d(v, sd[p + '._up_sample.weight'], sd[p + '._up_sample.bias'], stride=2) if up else v

    fx = unit(y_q, 'bottleneck', 0, True)
    for i in range(L):
        if concat:
            p = f'bridges_projection.{i}'
            b = norm_relu(bridges[i], p + '._bn1')
            b = norm_relu(F.conv2d(b, sd[p + '._c2.weight'], None, padding=1), p + '._bn2')
            fx = torch.cat((b, fx), dim=1)
        fx = unit(fx, f'synthesis_track.{i}', 1, i + 1 < L)
    return F.conv2d(fx, sd['fc.weight'], sd['fc.bias'])


def jnet_grad(sd, cfg, y_q, bridges, target, dtype=torch.float64):
    """-> (loss, {key: gradient}, logits) of the head with state dict `sd` in `dtype` on the CPU"""
    leaf = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    logits = jnet_forward(leaf, cfg, y_q.detach().cpu().to(dtype), [b.detach().cpu().to(dtype) for b in bridges])
    loss = head_loss(logits, target)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach() for k, v in leaf.items()}, logits.detach()


def rule_bound(f32, f64):
    """the rule of the head, per tensor: max|got - f64| <= 4 max|f32 restatement - f64| + 1e-6 max|f64|"""
    return 4.0 * float((f32.double() - f64.double()).abs().max()) + 1e-6 * float(f64.double().abs().max())


def rule_ratio(got, f32, f64):
    got = torch.as_tensor(got).detach().cpu().double()
    assert got.shape == f64.shape, (got.shape, f64.shape)
    assert bool(torch.isfinite(got).all())
    return float((got - f64.double()).abs().max()) / max(rule_bound(f32, f64), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulation of the backward kernels
def _f32(v):
    return np.asarray(v, dtype=np.float32)


def staged_np(x, a, b):
    """v = max(fmaf(a, x, b), 0) as fp32 (x (n, c, h, w), a / b (n, c))"""
    return SR.staged(torch.as_tensor(x), torch.as_tensor(a), torch.as_tensor(b)).numpy().astype(np.float32)


def wgrad_splits(n, h, w, cin, cout, ks):
    """the split rule of cae_seg_wgrad: (segments, steps per segment, steps per row)"""
    xs = (w + 15) // 16
    steps = n * h * xs
    tiles = ((cout + 31) // 32) * ((cin + 31) // 32)
    k = min((512 + tiles - 1) // tiles, max(1, steps // 16), 1024)
    per = (steps + k - 1) // k
    return (steps + per - 1) // per, per, xs


def wgrad_operands(g, srcs, ks, defect=None):
    """-> ((gh, gl), (vh, vl), padded v) float64 split operands of the weight gradient; srcs: staged fp32 sources"""
    v = np.concatenate([_f32(s) for s in srcs], axis=1)
    if defect == 'b_from_a' and len(srcs) == 2:
        v = np.concatenate([_f32(srcs[0]), _f32(srcs[0])[:, :srcs[1].shape[1]]], axis=1)
    return SR._split(g), SR._split(v)


def _corr(g, v, ks, border=None):
    """gw[co][ci][ky][kx] = sum g[n,co,y,x] v[n,ci,y+ky-P,x+kx-P] in float64; border (n, ci): the value outside the
    plane instead of zero (a planted defect)"""
    P = ks // 2
    vp = np.pad(v, ((0, 0), (0, 0), (P, P), (P, P)))
    if border is not None and P:
        edge = np.ones(vp.shape[2:], bool)
        edge[P:-P, P:-P] = False
        vp = np.where(edge[None, None], np.asarray(border, np.float64)[:, :, None, None], vp)
    h, w = g.shape[2:]
    out = np.zeros((g.shape[1], v.shape[1], ks, ks))
    for ky in range(ks):
        for kx in range(ks):
            out[:, :, ky, kx] = np.einsum('noyx,niyx->oi', g, vp[:, :, ky:ky + h, kx:kx + w])
    return out


def wgrad_replay(g, srcs, ks):
    """float64 replay of the f16x3 products on the split operands, and S = sum |g| |v|"""
    (gh, gl), (vh, vl) = wgrad_operands(g, srcs, ks)
    ref = _corr(gh, vh, ks) + _corr(gh, vl, ks) + _corr(gl, vh, ks)
    v = np.concatenate([_f32(s) for s in srcs], axis=1).astype(np.float64)
    return ref, _corr(np.abs(_f32(g).astype(np.float64)), np.abs(v), ks)


def emu_wgrad(g, srcs, ks, defect=None, border=None):
    """cae_seg_wgrad in the kernel's order: per pixel segment an fp32 partial, the partials merged in segment order in
    double and rounded once.  (Inside a segment the sum is wide: the fp32 accumulation is what C_CONV allows for.)"""
    g = _f32(g)
    n, cout, h, w = g.shape
    if defect == 'group_of_four_clipped' and w % 8 == 4:
        # a vectorised row whose second 16-byte group is taken only where the whole 8-pixel half lies inside: the row's last
        # four pixels of g read as zero (v's are then multiplied by nothing; its halo pixels are read one by one)
        g = g.copy()
        g[..., -4:] = 0
    (gh, gl), (vh, vl) = wgrad_operands(g, srcs, ks, defect)
    if defect == 'padding_counted':  # the pixels right of a ragged last step taken from the row's last pixel
        gh, gl = (np.concatenate([t, t[..., -1:]], axis=3) for t in (gh, gl))
        vh, vl = (np.pad(t, ((0, 0), (0, 0), (0, 0), (0, 1))) for t in (vh, vl))
        w += 1
    segs, per, xs = wgrad_splits(n, h, w, vh.shape[1], cout, ks)
    step = (np.arange(n)[:, None, None] * h + np.arange(h)[None, :, None]) * xs + (np.arange(w) // 16)[None, None, :]
    total = np.zeros((cout, vh.shape[1], ks, ks))
    for s in range(segs - 1 if defect == 'last_segment_dropped' else segs):
        mask = (step // per == s)[:, None].astype(np.float64)
        bh, bl = (None, None) if border is None else SR._split(border)
        part = _corr(gh * mask, vh, ks, bh) + _corr(gh * mask, vl, ks, bl) + _corr(gl * mask, vh, ks, bh)
        total += part.astype(np.float32).astype(np.float64)
    out = total.astype(np.float32)
    if defect == 'cico_swapped':
        out = np.ascontiguousarray(out.transpose(1, 0, 2, 3))
    return out


def emu_data_grad(g, w, defect=None):
    """the data gradient of a stride-1 convolution with weight w (cout, cin, k, k): cae_seg_conv2d on the flipped,
    transposed weight"""
    wd = _f32(w) if defect == 'no_flip' else _f32(w)[:, :, ::-1, ::-1]
    return SR.emu_conv([_f32(g)], np.ascontiguousarray(wd.transpose(1, 0, 2, 3)))


def emu_norm_relu_backward(x, a, b, gamma, gv, defect=None):
    """cae_seg_norm_relu_backward -> (g_x, dgamma, dbeta) fp32: statistics in two passes with double accumulators, the
    plane sums in double, the elementwise pass in fp32"""
    x, gv = _f32(x), _f32(gv)
    n, c, h, w = x.shape
    hw = h * w
    t = (_f32(a).astype(np.float64)[:, :, None, None] * x + _f32(b).astype(np.float64)[:, :, None, None]).astype(np.float32)
    mask = (x > 0) if defect == 'mask_from_x' else (t > 0)
    gu = np.where(mask, gv, np.float32(0))
    if gamma is None:
        return gu, None, None
    axes = (0, 2, 3) if defect == 'shared_stats' else (2, 3)
    cnt = n * hw if defect == 'shared_stats' else hw
    mf = (x.astype(np.float64).sum(axis=axes, keepdims=True) / cnt).astype(np.float32)
    e = x - mf
    m2 = (e * e).astype(np.float64).sum(axis=axes, keepdims=True)
    var = (m2 / (cnt - 1 if defect == 'unbiased' and cnt > 1 else cnt)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(var + np.float32(EPS), dtype=np.float32)).astype(np.float32)
    xh = (e * rstd).astype(np.float32)
    sg = gu.astype(np.float64).sum(axis=(2, 3), keepdims=True)
    sgx = (gu.astype(np.float64) * xh.astype(np.float64)).sum(axis=(2, 3), keepdims=True)
    mg = np.zeros_like(sg, dtype=np.float32) if defect == 'no_mean_g' else (sg / hw).astype(np.float32)
    mgx = np.zeros_like(sgx, dtype=np.float32) if defect == 'no_mean_gx' else (sgx / hw).astype(np.float32)
    coef = (_f32(gamma)[None, :, None, None] * rstd).astype(np.float32)
    if defect == 'stale_tail':  # a plane's elements from index 1024 on (its later blocks) see zero plane means
        tail = (np.arange(hw) >= 1024).reshape(1, 1, h, w)
        mg, mgx = np.where(tail, np.float32(0), mg), np.where(tail, np.float32(0), mgx)
    inner = ((gu - mg).astype(np.float32).astype(np.float64) - xh.astype(np.float64) * mgx).astype(np.float32)
    gx = (coef * inner).astype(np.float32)
    return gx, sgx.sum(axis=0).ravel().astype(np.float32), sg.sum(axis=0).ravel().astype(np.float32)


def emu_channel_sums(g, defect=None):
    """cae_seg_channel_sums: plane sums in double, the samples added in order, rounded once; 'one_block': the channels of
    the second and later 256-thread blocks of seg_channel_sums_kernel are left at zero"""
    g = _f32(g)
    out = g.reshape(g.shape[0], g.shape[1], -1).astype(np.float64).sum(axis=2).sum(axis=0).astype(np.float32)
    if defect == 'one_block':
        out[256:] = 0
    return out


def mask_margin(x, a, b):
    """the elements whose |a x + b| < 2^-20 (|a x| + |b|): there the mask of the fp32 fma may differ from float64's"""
    ax = torch.as_tensor(a).double()[:, :, None, None] * torch.as_tensor(x).double()
    bb = torch.as_tensor(b).double()[:, :, None, None]
    return (ax + bb).abs() < 2.0 ** -20 * (ax.abs() + bb.abs())


def norm_relu_backward_ref(x, a, b, gamma, beta, gv):
    """float64 reference of v = relu(GN(x)) backward on the fp32 inputs -> (g_x, dgamma, dbeta, margin): `margin` marks
    the elements whose |a x + b| < 2^-20 (|a x| + |b|), where the mask is allowed to differ"""
    xd = torch.as_tensor(x).double().requires_grad_(True)
    gd = None if gamma is None else torch.as_tensor(gamma).double().requires_grad_(True)
    bd = None if gamma is None else torch.as_tensor(beta).double().requires_grad_(True)
    v = torch.relu(xd if gamma is None else group_norm(xd, gd, bd))
    v.backward(torch.as_tensor(gv).double())
    margin = mask_margin(x, a, b)
    return xd.grad, None if gamma is None else gd.grad, None if gamma is None else bd.grad, margin


def norm_relu_backward_ref32(x, gamma, beta, gv):
    """the float32 restatement of the same backward (the yardstick of the rule) -> (g_x, dgamma, dbeta)"""
    xd = torch.as_tensor(x).float().clone().requires_grad_(True)
    gd = None if gamma is None else torch.as_tensor(gamma).float().clone().requires_grad_(True)
    bd = None if gamma is None else torch.as_tensor(beta).float().clone().requires_grad_(True)
    torch.relu(xd if gamma is None else group_norm(xd, gd, bd)).backward(torch.as_tensor(gv).float())
    return xd.grad, None if gamma is None else gd.grad, None if gamma is None else bd.grad


# ---------------------------------------------------------------------------------------------------------------------
# the whole backward in the kernels' order
# JNetTrain._backward brings every stage's gradient to max|G| in [2^(G_EXP - 1), 2^G_EXP) and the weight of every data
# gradient to max|w| in [2^(W_EXP - 1), 2^W_EXP) (seg_train.WEIGHT_EXP; None: the weight as it is, a planted defect)
G_EXP, W_EXP = 1, 15


def plan_of(cfg):
    """JNet.stage_plan() from the constructor keys: dict(name, ks, up, norm (prefix or None), srcs)"""
    L, concat = cfg['compression_level'], cfg.get('concat_bridges', False)
    plan = []

    def add(name, ks, srcs, norm=None, up=False):
        plan.append(dict(name=name, ks=ks, up=up, norm=norm, srcs=srcs))
        return len(plan) - 1

    s = add('bottleneck._c1', 1, [('latent',)], 'bottleneck._bn1')
    s = add('bottleneck._c2', 3, [('raw', s, True)], 'bottleneck._bn2')
    up = add('bottleneck._up_sample', 1, [('raw', s, True)], up=True)
    for i in range(L):
        srcs = [('raw', up, False)]
        if concat:
            s = add(f'bridges_projection.{i}._c2', 3, [('bridge', i)], f'bridges_projection.{i}._bn2')
            srcs = [('raw', s, True)] + srcs
        s = add(f'synthesis_track.{i}._c1', 3, srcs, f'synthesis_track.{i}._bn1')
        s = add(f'synthesis_track.{i}._c2', 3, [('raw', s, True)], f'synthesis_track.{i}._bn2')
        if i + 1 < L:
            up = add(f'synthesis_track.{i}._up_sample', 1, [('raw', s, True)], up=True)
    add('fc', 1, [('raw', s, True)])
    return plan


def _plane_ab(x, gamma, beta):
    """(a, b) (n, c) fp32 of GroupNorm(C) from float64 statistics of the fp32 planes; gamma None: (1, 0)"""
    n, c = x.shape[:2]
    if gamma is None:
        return np.ones((n, c), np.float32), np.zeros((n, c), np.float32)
    xd = np.asarray(x, np.float64)
    m = xd.mean(axis=(2, 3))
    var = ((xd - m[:, :, None, None]) ** 2).mean(axis=(2, 3))
    a = (np.asarray(gamma, np.float64)[None] / np.sqrt(var + EPS)).astype(np.float32)
    return a, (np.asarray(beta, np.float64)[None] - m * a).astype(np.float32)


def _unshuffle(g, defect=None):
    n, c, h, w = g.shape
    g = g.reshape(n, c, h // 2, 2, w // 2, 2)
    g = g.transpose(0, 1, 5, 3, 2, 4) if defect == 'parity_swapped' else g.transpose(0, 1, 3, 5, 2, 4)
    return np.ascontiguousarray(g.reshape(n, c * 4, h // 2, w // 2))


def emu_backward(cfg, sd, y_q, bridges, target, defect=None, g_exp=G_EXP, w_exp=W_EXP):
    """-> (loss, {key: gradient}): forward by the float32 restatement, backward through the emulated operations in the
    order of JNetTrain._backward, every stage's gradient and every data gradient's weight renormalised by a power of two"""
    bn = cfg.get('batch_norm', True)
    logits, stages = SR.jnet(sd, cfg, y_q, bridges, torch.float32)
    lg = logits.clone().requires_grad_(True)
    loss = head_loss(lg, target)
    loss.backward()
    plan = plan_of(cfg)
    par = {k: v.numpy() for k, v in sd.items()}
    raw = [stages[st['name']].numpy() for st in plan]
    ab = [(_plane_ab(raw[k], par.get(st['norm'] + '.weight') if bn else None, par.get(st['norm'] + '.bias') if bn else None)
           if st['norm'] else None) for k, st in enumerate(plan)]
    out = {}
    graw = {len(plan) - 1: (lg.grad.numpy().astype(np.float32), 1.0)}

    def source(src):
        if src[0] == 'latent':
            return y_q.numpy(), None, False, None
        if src[0] == 'bridge':
            p = f'bridges_projection.{src[1]}._bn1'
            x = bridges[src[1]].numpy()
            return x, _plane_ab(x, par[p + '.weight'] if bn else None, par[p + '.bias'] if bn else None), bn, p
        return raw[src[1]], (ab[src[1]] if src[2] else None), True, (plan[src[1]]['norm'] if bn and src[2] else None)

    for k in reversed(range(len(plan))):
        st, (G, cum) = plan[k], graw.pop(k)
        mx = float(np.abs(G).max())
        sk = 2.0 ** (g_exp - np.frexp(mx)[1])
        G, cum = (G * np.float32(sk)).astype(np.float32), cum * sk
        keep = 1.0 if defect == 'scale_kept' else 1.0 / cum
        name, w = st['name'], par[st['name'] + '.weight']
        srcs = [source(sr) for sr in st['srcs']]
        vs = [x if t is None else staged_np(x, *t) for x, t, _, _ in srcs]
        if name + '.bias' in par:
            taps = (4 if st['up'] else st['ks'] ** 2) if defect == 'bias_per_tap' else 1
            out[name + '.bias'] = (G.astype(np.float64).sum(axis=(0, 2, 3)) * taps).astype(np.float32) * np.float32(keep)
        wmax = float(np.abs(w).max())
        sw = 1.0 if w_exp is None else 2.0 ** (w_exp - np.frexp(wmax)[1])  # the data gradient's weight, scaled likewise
        if st['up']:
            G = _unshuffle(G, defect)
            cin, cout = w.shape[:2]
            gw = emu_wgrad(G, vs, 1).reshape(cout, 2, 2, cin).transpose(3, 0, 1, 2)
            wd = w.reshape(cin, 4 * cout, 1, 1)
            gv = SR.emu_conv([G], wd * np.float32(sw))
        else:
            gw = emu_wgrad(G, vs, st['ks'], defect)
            if gw.shape != w.shape:  # (the swapped defect on a non-square layer)
                gw = np.zeros_like(w)
            gv = emu_data_grad(G, w * np.float32(sw), defect)
        out[name + '.weight'] = np.ascontiguousarray(gw) * np.float32(keep)
        if not any(sr[2] for sr in srcs):
            continue
        gv, c0 = gv.astype(np.float32), 0
        cum = cum * sw
        keep = 1.0 if defect == 'scale_kept' else 1.0 / cum
        for sr, (x, t, want, norm) in zip(st['srcs'], srcs):
            piece = gv[:, c0:c0 + x.shape[1]]
            c0 += x.shape[1]
            if not want:
                continue
            if t is None:
                graw[sr[1]] = (piece, cum)
                continue
            gx, dg, db = emu_norm_relu_backward(x, t[0], t[1], par[norm + '.weight'] if norm else None, piece, defect)
            if norm:
                out[norm + '.weight'], out[norm + '.bias'] = dg * np.float32(keep), db * np.float32(keep)
            if sr[0] != 'bridge':
                graw[sr[1]] = (gx, cum)
    return float(loss.detach()), {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}
