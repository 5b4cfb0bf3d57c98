"""Per-operation replay of the composed training path (train._composed_track).

`record()` wraps `.apply` of the small autograd functions a composed track is made of -- _ConvS1Fn, _ConvS2Fn, single-layer
SynthesisFn, _GdnFn, _BatchNormFn, _ColourFn -- for the duration of a `with` block.  For every call it keeps the inputs the
function received on the GPU, its outputs, the gradient it was handed and the gradients it returned (identity taps around
the call: values and the autograd graph are unchanged).  `replay()` then recomputes every operation alone, in float64 on
the CPU, from those same inputs and handed gradients, with the rounding points of the kernels (bf16 operands of every
convolution, bf16 gradients into weight / data gradients, bf16 GDN outputs and data gradients), and judges each result
locally:

  * fp32 results: |got - ref| <= c * 2^-24 * S + 1e-6 max|ref|, S = the sum of the magnitudes of the terms (the same
    operation on |operands|), c = 32 -- condition-aware, so an ill-conditioned sum is neither failed nor excused;
  * results rounded to bf16: one bf16 ulp of the value on top of that.

Errors that grow along an ill-conditioned chain of operations do not enter the verdict: an operation that is wrong fails
locally, a model whose operations are all locally right passes.  LeakyReLU / ReLU mask disagreements between the kernel's
output and the float64 replay are allowed only where the float64 pre-activation is within the fp32 bound of 0; the replay
then follows the kernel's mask, and counts them.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
C32 = 32.0
# the colour layer's edge form carries its folded output gradient as a bf16 (hi, lo) pair: ~2^-17 of each folded value
# (include/cae_hip.h, cae_t_im2col_s1r) -> 2^7 x the fp32 constant on what is computed from it
C_COLOUR_EDGE = 256.0


class _Tap(torch.autograd.Function):
    """identity; its backward stores the gradient passing through under rec[key][slot]"""

    @staticmethod
    def forward(ctx, x, rec, key, slot):
        ctx.rec, ctx.key, ctx.slot = rec, key, slot
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.rec.setdefault(ctx.key, {})[ctx.slot] = None if g is None else g.detach().double().cpu()
        return g, None, None, None


def _kind(fn, args):
    from cnn_autoencoder_amd import train
    if fn is train.SynthesisFn and (len(args[1]) != 1 or args[2]):
        return None  # (a fused track: not part of a composed one)
    return {train._ConvS1Fn: 'conv_s1', train._ConvS2Fn: 'conv_s2', train.SynthesisFn: 'synthesis', train._GdnFn: 'gdn',
            train._BatchNormFn: 'bn', train._ColourFn: 'colour'}[fn]


@contextlib.contextmanager
def record():
    """with record() as calls: run forward and backward of a composed track; calls = [dict(kind, args, out, gin, gout)]"""
    from cnn_autoencoder_amd import train
    classes = [train._ConvS1Fn, train._ConvS2Fn, train.SynthesisFn, train._GdnFn, train._BatchNormFn, train._ColourFn]
    calls: List[dict] = []
    saved = {cls: cls.__dict__.get('apply') for cls in classes}

    def make(cls, orig):
        def apply(*args):
            kind = _kind(cls, args)
            if kind is None:
                return orig(*args)
            rec = dict(kind=kind, args=[a.detach().double().cpu() if torch.is_tensor(a) else a for a in args])
            tapped = [(_Tap.apply(a, rec, 'gin', i) if torch.is_tensor(a) and a.requires_grad else a) for i, a in enumerate(args)]
            out = orig(*tapped)
            outs = out if isinstance(out, tuple) else (out,)
            rec['out'] = [o.detach().double().cpu() for o in outs]
            calls.append(rec)
            outs = tuple(_Tap.apply(o, rec, 'gout', j) if o.requires_grad else o for j, o in enumerate(outs))
            return outs if isinstance(out, tuple) else outs[0]
        return apply

    for cls in classes:
        cls.apply = make(cls, cls.apply)
    try:
        yield calls
    finally:
        for cls in classes:
            if saved[cls] is None:
                del cls.apply
            else:
                cls.apply = saved[cls]


def bf(x):
    return x.bfloat16().double()


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


class Verdict:
    """per-quantity ratios err / bound (<= 1 passes), failures, mask disagreements"""

    def __init__(self):
        self.ratios: Dict[str, float] = {}
        self.failures: List[str] = []
        self.mask_flips = 0
        self.ops = 0

    def check(self, what, got, ref, S, ulp16=False, c=C32):
        got, ref, S = got.double(), ref.double(), S.double()
        if got.shape != ref.shape:
            self.failures.append(f'{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}')
            return
        err = (got - ref).abs()
        bound = c * U32 * S + 1e-6 * float(ref.abs().max()) + 1e-300
        if ulp16:
            bound = bound + bf16_ulp(ref)
        finite = bool(torch.isfinite(got).all())
        r = float((err / bound).max()) if finite else float('inf')
        self.ratios[what] = r
        if not r <= 1.0:
            self.failures.append(f'{what}: error {float(err.max()):.3e} is {r:.2f} x its bound')

    @property
    def worst(self) -> float:
        return max(self.ratios.values()) if self.ratios else 0.0

    def summary(self) -> str:
        return (f'{self.ops} operations, {len(self.ratios)} results, worst error / bound {self.worst:.3f}, '
                f'{self.mask_flips} activation-mask disagreements at |pre-activation| within rounding of 0, '
                f'{len(self.failures)} failures')


def _lin(fn, xs, g):
    """value, |terms| bound, and gradients (with their |terms| bounds) of a bilinear fn(*xs) against g"""
    leaves = [x.clone().requires_grad_(True) for x in xs]
    aleaves = [x.abs().requires_grad_(True) for x in xs]
    v = fn(*leaves)
    S = fn(*aleaves)
    grads = sgrads = None
    if g is not None:
        grads = torch.autograd.grad(v, leaves, g)
        sgrads = torch.autograd.grad(S, aleaves, g.abs())
    return v.detach(), S.detach(), grads, sgrads


def _act_mask(v, S, out_k, act, tag, V: Verdict):
    """the kernel's activation mask (out > 0), checked against the float64 pre-activation v"""
    mk = out_k > 0
    mr = v > 0
    flip = mk != mr
    near0 = v.abs() <= C32 * U32 * S + 1e-300
    bad = flip & ~near0
    if bool(bad.any()):
        V.failures.append(f'{tag}: {int(bad.sum())} activation-mask disagreements away from 0')
    V.mask_flips += int(flip.sum())
    return mk


def _replay_conv_s1(r, tag, V):
    x, synthesis, ks, act, w, b = r['args']
    P = ks // 2
    if synthesis:
        fn = lambda xx, ww: F.conv_transpose2d(xx, ww, padding=P)  # noqa: E731
    else:
        fn = lambda xx, ww: F.conv2d(F.pad(xx, (P,) * 4, mode='reflect'), ww)  # noqa: E731
    v, S, _, _ = _lin(fn, (bf(x), bf(w)), None)
    if b is not None:
        v, S = v + b.view(1, -1, 1, 1), S + b.abs().view(1, -1, 1, 1)
    out_k = r['out'][0]
    slope = 0.01 if act == 1 else 0.0
    if act:
        mk = _act_mask(v, S, out_k, act, tag, V)
        ref = torch.where(v > 0, v, slope * v)
    else:
        ref = v
    V.check(tag + ' out', out_k, ref, S)
    g = r.get('gout', {}).get(0)
    if g is None:
        return
    if act:  # (the kernel scales the fp32 gradient in fp32, then rounds: emulated exactly)
        gu = torch.where(mk, g.float(), g.float() * torch.tensor(slope, dtype=torch.float32)).bfloat16().double()
    else:
        gu = bf(g)
    _, _, (gx, gw), (Sgx, Sgw) = _lin(fn, (bf(x), bf(w)), gu)
    gin = r.get('gin', {})
    if 4 in gin:
        V.check(tag + ' grad w', gin[4], gw, Sgw)
    if b is not None and 5 in gin:
        V.check(tag + ' grad b', gin[5], gu.sum(dim=(0, 2, 3)), gu.abs().sum(dim=(0, 2, 3)))
    if 0 in gin:
        V.check(tag + ' grad x', gin[0], gx, Sgx, ulp16=not synthesis)  # (analysis: folded into bf16)


def _replay_conv_s2(r, tag, V):
    x, ks, w, b = r['args']
    P = ks // 2
    fn = lambda xx, ww: F.conv2d(F.pad(xx, (P,) * 4, mode='reflect'), ww, stride=2)  # noqa: E731
    g = r.get('gout', {}).get(0)
    g16 = None if g is None else bf(g)
    v, S, grads, sgrads = _lin(fn, (bf(x), bf(w)), g16)
    if b is not None:
        v, S = v + b.view(1, -1, 1, 1), S + b.abs().view(1, -1, 1, 1)
    V.check(tag + ' out', r['out'][0], v, S)
    if g16 is None:
        return
    gin = r.get('gin', {})
    if 2 in gin:
        V.check(tag + ' grad w', gin[2], grads[1], sgrads[1])
    if b is not None and 3 in gin:
        V.check(tag + ' grad b', gin[3], g16.sum(dim=(0, 2, 3)), g16.abs().sum(dim=(0, 2, 3)))
    if 0 in gin:
        V.check(tag + ' grad x', gin[0], grads[0], sgrads[0], ulp16=True)


def _replay_synthesis(r, tag, V):
    x, specs, _colour = r['args'][:3]
    s = specs[0]
    w = r['args'][3]
    b = r['args'][4] if s.has_bias else None
    P = s.ks // 2
    fn = lambda xx, ww: F.conv_transpose2d(xx, ww, stride=2, padding=P, output_padding=1)  # noqa: E731
    g = r.get('gout', {}).get(0)
    g16 = None if g is None else bf(g)
    v, S, grads, sgrads = _lin(fn, (bf(x), bf(w)), g16)
    if b is not None:
        v, S = v + b.view(1, -1, 1, 1), S + b.abs().view(1, -1, 1, 1)
    V.check(tag + ' out', r['out'][0], v, S)
    if g16 is None:
        return
    gin = r.get('gin', {})
    if 3 in gin:
        V.check(tag + ' grad w', gin[3], grads[1], sgrads[1])
    if b is not None and 4 in gin:
        V.check(tag + ' grad b', gin[4], g16.sum(dim=(0, 2, 3)), g16.abs().sum(dim=(0, 2, 3)))
    if 0 in gin:
        V.check(tag + ' grad x', gin[0], grads[0], sgrads[0])


def _replay_gdn(r, tag, V):
    x, inverse, beta_p, gamma_p = r['args']
    c = x.shape[1]
    beta, gamma = beta_p[:c], gamma_p[:c, :c]
    z = x  # (fp32 values, kept in fp32 by the kernel)
    nrm = F.conv2d(z * z, gamma.reshape(c, c, 1, 1), beta)  # all terms >= 0: well conditioned
    e = 0.5 if inverse else -0.5
    f = nrm ** e
    y = z * f
    V.check(tag + ' out', r['out'][0], y, y.abs() * 4, ulp16=True)
    g = r.get('gout', {}).get(0)
    if g is None:
        return
    # y_c = z_c n_c^e:  t_c = g_c z_c e n_c^(e-1);  dz_j = g_j n_j^e + 2 z_j sum_c t_c gamma_cj;  dbeta_c = sum t_c;
    # dgamma_cj = sum t_c z_j^2
    t = g * z * e * nrm ** (e - 1)
    cross = torch.einsum('nchw,cj->njhw', t, gamma)
    Scross = torch.einsum('nchw,cj->njhw', t.abs(), gamma.abs())
    dz = g * f + 2 * z * cross
    Sdz = (g * f).abs() + 2 * z.abs() * Scross
    gin = r.get('gin', {})
    if 0 in gin:
        V.check(tag + ' grad x', gin[0], dz, Sdz, ulp16=True)
    if 2 in gin:
        V.check(tag + ' grad beta', gin[2][:c], t.sum(dim=(0, 2, 3)), t.abs().sum(dim=(0, 2, 3)))
    if 3 in gin:
        z2 = z * z
        V.check(tag + ' grad gamma', gin[3][:c, :c], torch.einsum('nchw,njhw->cj', t, z2),
                torch.einsum('nchw,njhw->cj', t.abs(), z2))


def bn_reference(x, weight, bias, eps, dy=None):
    """float64 nn.BatchNorm2d (batch statistics) on the fp32 input x and its |terms| bounds in the kernels' affine form:
    -> dict(y, Sy[, dx, Sdx, dw, Sdw, db, Sdb])"""
    c = x.shape[1]
    wt = weight if weight is not None else torch.ones(c, dtype=torch.float64)
    bs = bias if bias is not None else torch.zeros(c, dtype=torch.float64)
    xl = x.clone().requires_grad_(True)
    wl, bl = wt.clone().requires_grad_(True), bs.clone().requires_grad_(True)
    y = F.batch_norm(xl, None, None, wl, bl, True, 0.0, eps)
    mu = x.mean(dim=(0, 2, 3))
    rstd = (x.var(dim=(0, 2, 3), unbiased=False) + eps).rsqrt()
    A = (wt * rstd).view(1, -1, 1, 1)
    # y = x A + C in fp32, A and C rounded to fp32 once: a few 2^-24 of |x A| + |C|
    out = dict(y=y.detach(), Sy=(x * A).abs() + (bs.view(1, -1, 1, 1) - mu.view(1, -1, 1, 1) * A).abs())
    if dy is None:
        return out
    y.backward(dy)
    m = x.numel() / c
    xhat = (x - mu.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
    sdyx = (dy * xhat).sum(dim=(0, 2, 3))
    B = (-wt * rstd * rstd * sdyx / m).view(1, -1, 1, 1)
    C = (wt * rstd * (-dy.sum(dim=(0, 2, 3)) / m + mu * rstd * sdyx / m)).view(1, -1, 1, 1)
    # the weight gradient (sum dy xhat) comes from s2 - mean s1 of double sums: its fp32 rounding, and the double sums'
    # cancellation (2^-53 of |mean| sum |dy| rstd, far below)
    out.update(dx=xl.grad, Sdx=(dy * A).abs() + (x * B).abs() + C.abs(), dw=wl.grad, Sdw=(dy * xhat).abs().sum(dim=(0, 2, 3)),
               db=bl.grad, Sdb=dy.abs().sum(dim=(0, 2, 3)))
    return out


def _replay_bn(r, tag, V):
    x, weight, bias, eps = r['args']
    g = r.get('gout', {}).get(0)
    ref = bn_reference(x, weight, bias, eps, g)
    V.check(tag + ' out', r['out'][0], ref['y'], ref['Sy'], c=4.0)
    if g is None:
        return
    gin = r.get('gin', {})
    if 0 in gin:
        V.check(tag + ' grad x', gin[0], ref['dx'], ref['Sdx'], c=8.0)
    if 1 in gin:
        V.check(tag + ' grad weight', gin[1], ref['dw'], ref['Sdw'], c=4.0)
    if 2 in gin:
        V.check(tag + ' grad bias', gin[2], ref['db'], ref['Sdb'], c=4.0)


def _replay_colour(r, tag, V):
    from cnn_autoencoder_amd import train
    x, cs, w, b = r['args']
    P = cs.ks // 2
    fn = lambda xx, ww: F.conv2d(F.pad(xx, (P,) * 4, mode='reflect'), ww)  # noqa: E731
    g = r.get('gout', {}).get(0)
    g16 = None if g is None else bf(g)
    v, S, grads, sgrads = _lin(fn, (bf(x), bf(w)), g16)
    if b is not None:
        v, S = v + b.view(1, -1, 1, 1), S + b.abs().view(1, -1, 1, 1)
    V.check(tag + ' out', r['out'][0], v, S)
    if g16 is None:
        return
    c = C_COLOUR_EDGE if train._colour_edge(cs) else C32
    gin = r.get('gin', {})
    if 2 in gin:
        V.check(tag + ' grad w', gin[2], grads[1], sgrads[1], c=c)
    if b is not None and 3 in gin:
        V.check(tag + ' grad b', gin[3], g16.sum(dim=(0, 2, 3)), g16.abs().sum(dim=(0, 2, 3)))
    if 0 in gin:
        V.check(tag + ' grad x', gin[0], grads[0], sgrads[0], c=c)


_REPLAY = dict(conv_s1=_replay_conv_s1, conv_s2=_replay_conv_s2, synthesis=_replay_synthesis, gdn=_replay_gdn, bn=_replay_bn,
               colour=_replay_colour)


def replay(calls) -> Verdict:
    """the local float64 verdict of every recorded operation"""
    V = Verdict()
    for i, r in enumerate(calls):
        _REPLAY[r['kind']](r, f'op {i} {r["kind"]}', V)
        V.ops += 1
    return V


def colour_leaves(dec, n_levels):
    """[(weight, bias | None)] leaves of a multiscale decoder's colour layers (grouped ones as their dense block-diagonal
    embedding, differentiable) and their [(parameter name, leaf)]"""
    cols, pairs = [], []
    for i in range(n_levels - 1):
        conv = dec.color_layers[i][0]
        w = conv.weight.detach().cpu().clone().requires_grad_(True)
        pairs.append((f'color_layers.{i}.0.weight', w))
        b = None
        if conv.bias is not None:
            b = conv.bias.detach().cpu().clone().requires_grad_(True)
            pairs.append((f'color_layers.{i}.0.bias', b))
        if conv.groups > 1:
            cout_g = conv.out_channels // conv.groups
            w = torch.block_diag(*[w[j * cout_g:(j + 1) * cout_g].reshape(cout_g, -1) for j in range(conv.groups)]).reshape(
                conv.out_channels, conv.in_channels, *conv.weight.shape[2:])
        cols.append((w, b))
    return cols, pairs


def restate(x, units, colours, synthesis, bf16):
    """the restatement of a track -> list of outputs: [x_r, colour_{L-2} .. colour_0] with colour layers, else [y].  Colour
    layer: reflect-padded F.conv2d of the level's output, bf16 operands, bf16-rounded output gradient (as _ColourFn)."""
    from oracle import train_oracle as T
    levels = T.residual_track(x, units, synthesis, bf16=bf16, levels=True)
    cols = []
    for i, (w, b) in enumerate(colours):
        k = w.shape[-1]
        cols.append(T._g(F.conv2d(F.pad(T._r(levels[i], bf16), (k // 2,) * 4, mode='reflect'), T._r(w, bf16), b), bf16))
    return [levels[-1]] + cols[::-1]


def judge_track(mod, track, inp, synthesis, act_name, limit=None):
    """Forward + backward of one track (a multiscale decoder: with its colour layers) on the GPU under record(), against the
    restatement with the kernels' rounding points (bf16) and without them in float64 (a float64 copy of the modules).
    -> (Verdict of the per-operation replay, rows), rows = [(name, distance of the GPU result from the float64 one, distance
    of the bf16 restatement's from it, the largest float64 gradient of the parameter's unit, the float64 result's own largest
    magnitude)] for every parameter gradient, every output ('out i') and the latent gradient ('latent') -- distances as
    max |difference|.  `limit`: (None, None) when the bf16 restatement's outputs are not finite or exceed it (an untrained
    residual / IGDN stack can blow up in the restatement itself)."""
    import copy
    from conftest import residual_oracle_units
    for p in mod.parameters():
        p.grad = None  # (the gradients read below are this call's alone)
    ms = synthesis and getattr(mod, 'multiscale_analysis', False)
    L = len(track)
    units, pairs = residual_oracle_units(track, act_name)
    colours, cpairs = colour_leaves(mod, L) if ms else ([], [])
    mod64 = copy.deepcopy(mod).cpu().double()
    track64 = mod64.synthesis_track if synthesis else mod64.analysis_track
    units64, pairs64 = residual_oracle_units(track64, act_name)
    colours64, cpairs64 = colour_leaves(mod64, L) if ms else ([], [])
    xin = inp.clone().requires_grad_(synthesis)
    ref = restate(xin, units, colours, synthesis, True)
    if limit is not None and not all(bool(torch.isfinite(r).all()) and float(r.detach().abs().max()) <= limit for r in ref):
        return None, None
    g = [torch.randn_like(r.detach()) for r in ref]  # (the sweep's draw order: right after the restatement's forward)
    torch.autograd.backward(ref, g)
    x64 = inp.double().requires_grad_(synthesis)
    ref64 = restate(x64, units64, colours64, synthesis, False)
    torch.autograd.backward(ref64, [t.double() for t in g])
    xdev = inp.cuda().requires_grad_(synthesis)
    with record() as calls:
        out = mod(xdev)
        outs = [t for t in out[0] if t is not None] if synthesis else [out]
        assert len(outs) == len(ref)
        torch.autograd.backward(outs, [t.cuda() for t in g])
    V = replay(calls)
    got = {k: p.grad.detach().double().cpu() for k, p in mod.named_parameters() if p.grad is not None}
    prefix = 'synthesis_track.' if synthesis else 'analysis_track.'
    named = [(prefix + n, lb, l64) for (n, lb), (_, l64) in zip(pairs, pairs64)] + \
        [(n, lb, l64) for (n, lb), (_, l64) in zip(cpairs, cpairs64)]
    if len(got) != len(named):
        raise AssertionError(f'{len(got)} gradients for {len(named)} parameters')
    unit = lambda name: '.'.join(name.split('.')[:2])  # noqa: E731  (track.i / color_layers.i)
    unit_max: Dict[str, float] = {}
    for name, _, l64 in named:
        unit_max[unit(name)] = max(unit_max.get(unit(name), 0.0), float(l64.grad.abs().max()))
    dist = lambda a, b: float((a.double() - b.double()).abs().max())  # noqa: E731
    rows = []
    for name, lb, l64 in named:
        rows.append((name, dist(got[name], l64.grad), dist(lb.grad, l64.grad), unit_max[unit(name)],
                     float(l64.grad.abs().max())))
    for i, (o, r, r64) in enumerate(zip(outs, ref, ref64)):
        m = float(r64.detach().abs().max())
        rows.append((f'out {i}', dist(o.detach().cpu(), r64.detach()), dist(r.detach(), r64.detach()), max(1.0, m), m))
    if synthesis:
        m = float(x64.grad.abs().max())
        rows.append(('latent', dist(xdev.grad.cpu(), x64.grad), dist(xin.grad, x64.grad), m, m))
    return V, rows


# End-to-end bound of each gradient / output against the float64 restatement: a multiple of the distance of the restatement
# WITH the kernels' rounding points from it (what the roundings alone cost this result), plus a floor relative to the largest
# gradient of the parameter's unit (a parameter whose float64 gradient is near zero next to its unit's carries only noise).
# Observed on an MI355X for the four one-channel cases the old sweep flagged: the GPU's distance is 1.0 - 2.1 x the
# restatement's for all but three gradients, which lie at 9.6 x (3:167 0.res_model.0.bias: 4.7e-3 of its unit's largest
# gradient), 8.5 x (3:93 0.model.1.weight: 1.3e-3) and 40 x (5:84 0.res_model.1.bias: 1.1e-3) -- while every operation of
# those tracks passes its local float64 bound: two summation orders of the same roundings through an ill-conditioned chain.
E2E_MULTIPLE, E2E_FLOOR = 4.0, 1e-2


def e2e_rule(row):
    """-> 'multiple' (within E2E_MULTIPLE x the restatement's distance), 'floor' (only within the floor added) or 'fail'"""
    _, e_k, e_b, unit_max, _ = row
    if e_k <= E2E_MULTIPLE * e_b:
        return 'multiple'
    return 'floor' if e_k <= E2E_MULTIPLE * e_b + E2E_FLOOR * unit_max else 'fail'
