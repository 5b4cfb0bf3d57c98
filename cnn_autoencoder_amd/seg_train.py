"""Training the compressed-domain segmentation head: the reference trains ``seg_model`` with the codec frozen
(``_taskutils.py:46-110``) under the ``BCEWithLogits`` / ``CrossEntropy`` losses of ``criteria/_classification.py``.

``JNetTrain`` is ``segmenters.JNet`` with a backward pass.  Without autograd the forward is the inference head's one
library call; under autograd it walks ``stage_plan()`` over ``cae_seg_conv2d`` with every weight scaled by a power of two
before the f16 split (``_forward_taps``) and keeps every stage's raw output and (a, b) pair; the backward walks the plan in
reverse over per-operation entry points on NCHW fp32 tensors (csrc/cae_seg_train.hip, csrc/cae_kernels_seg_train.hpp):

    cae_seg_wgrad               weight gradients, f16x3 on the MFMA with the contraction over pixels
    cae_seg_conv2d              data gradients: the forward kernel on the flipped, transposed weight
    cae_seg_norm_relu_backward  GroupNorm(one group per channel) + ReLU, with gamma / beta gradients
    cae_seg_channel_sums        bias gradients

Pixel-unshuffling a gradient, flipping / transposing a weight and splitting a concatenated gradient stay torch ops on the
device.  ``y_q`` and the bridges are constants: joint training of codec and head is not built.

Gradient scale.  The f16x3 kernels need |v| <= 65504 and lose relative precision below about 6e-5, and the logit
gradients of a mean-reduced loss are far smaller.  The backward is linear in g_logits, so it reads m = max|g_logits| once
(the step's one synchronisation) and propagates s g with s = 2^-floor(log2 m).
One scale per step does not suffice: without normalisation the gradients shrink stage by stage until their small entries
fall into the f16 subnormals (the 'nobn' golden configuration missed its bound by 1.8 on the first projection's weight).
So every stage's gradient is brought back to max|G| in [1, 2) by a further power of two, computed and applied on the
device with no further synchronisation, and every parameter gradient is multiplied by the inverse of the scale it was
computed under; all these multiplications are exact.  The weight of every data gradient is scaled the same way, to
max|w| in [2^14, 2^15): the low half of an f16 split below 2^-14 is subnormal, so a weight near 0.01 (the canonical
widths) kept 2^-18 of itself instead of 2^-22, and the canonical head missed its bound by 1.41 until this was done here and in the training forward.
A staged value of the backward outside
the f16 range raises a device word that ``JNetTrain.check_backward()`` / ``train_step`` read (FloatingPointError).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import segmenters
from .segmenters import JNet

JOINT = ('joint training of codec and segmentation head is not built: y_q and the bridges are constants of the head '
         '(detach them, or run the codec under torch.no_grad() as seg_train.setup_forward_func does)')


# ---- one wrapper per entry point ---------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max((int(nbytes) + 7) // 8, 1), dtype=torch.int64, device=dev)


def _f32(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.float32:
        raise ValueError('expected an fp32 tensor on the device')
    return t.contiguous()


def new_flag(dev) -> torch.Tensor:
    """the zeroed overflow word the backward entry points raise"""
    return torch.zeros(1, dtype=torch.int32, device=dev)


def pack_dev(w: torch.Tensor, cin_a: int, cin_b: int, cout: int, ks: int, up: bool, flag: Optional[torch.Tensor] = None):
    """cae_seg_pack_dev: device fp32 weight -> device halves (int16 tensor), byte for byte cae_seg_pack's"""
    w = _f32(w)
    L = _lib.lib()
    n = int(L.cae_seg_packed_halves(cin_a, cin_b, cout, ks, int(up)))
    out = torch.empty(max(n, 1), dtype=torch.int16, device=w.device)
    _lib.check(L.cae_seg_pack_dev(w.data_ptr(), cin_a, cin_b, cout, ks, int(up), out.data_ptr(), n, _ptr(flag),
                                  _lib.stream_ptr()))
    return out[:n]


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], flag: torch.Tensor,
           ab: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cae_seg_conv2d: stride-1 zero-padded convolution (ks 1 or 3) of x (or of max(fmaf(a, x, b), 0)) with w"""
    x, w = _f32(x), _f32(w)
    n, cin, h, wd = x.shape
    cout, ks = w.size(0), w.size(2)
    if w.size(1) != cin or w.size(3) != ks:
        raise ValueError(f'weight {tuple(w.shape)} does not fit an input of {cin} channels')
    L = _lib.lib()
    out = torch.empty((n, cout, h, wd), dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    ws = _ws(L.cae_seg_conv2d_workspace(n, cin, cout, h, wd, ks), x.device)
    _lib.check(L.cae_seg_conv2d(x.data_ptr(), _ptr(ab), w.data_ptr(), _ptr(None if bias is None else _f32(bias)), n, cin,
                                cout, h, wd, ks, out.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                _lib.stream_ptr()))
    return out


def wgrad(g: torch.Tensor, srcs: Sequence, ks: int, flag: torch.Tensor) -> torch.Tensor:
    """cae_seg_wgrad: g (n, cout, h, w); srcs: one or two (x, ab or None) -> gw (cout, cin_a + cin_b, ks, ks)"""
    g = _f32(g)
    n, cout, h, wd = g.shape
    (xa, aba), (xb, abb) = srcs[0], (srcs[1] if len(srcs) > 1 else (None, None))
    xa = _f32(xa)
    xb = None if xb is None else _f32(xb)
    ca, cb = xa.size(1), 0 if xb is None else xb.size(1)
    for x in (xa, xb):
        if x is not None and (x.size(0), x.size(2), x.size(3)) != (n, h, wd):
            raise ValueError(f'source {tuple(x.shape)} does not fit a gradient {tuple(g.shape)}')
    L = _lib.lib()
    gw = torch.empty((cout, ca + cb, ks, ks), dtype=torch.float32, device=g.device)
    if n == 0:
        return gw.zero_()
    ws = _ws(L.cae_seg_wgrad_workspace(n, h, wd, ca + cb, cout, ks), g.device)
    _lib.check(L.cae_seg_wgrad(g.data_ptr(), xa.data_ptr(), _ptr(aba), ca, _ptr(xb), _ptr(abb), cb, n, cout, h, wd, ks,
                               gw.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr()))
    return gw


def norm_relu_backward(x: torch.Tensor, ab: torch.Tensor, gamma: Optional[torch.Tensor], gv: torch.Tensor,
                       need_gx: bool = True):
    """cae_seg_norm_relu_backward -> (g_x or None, dgamma or None, dbeta or None)"""
    x, gv = _f32(x), _f32(gv)
    n, c = x.shape[:2]
    hw = x[0, 0].numel() if n else 1
    L = _lib.lib()
    gx = torch.empty_like(x) if need_gx else None
    if gamma is None:
        _lib.check(L.cae_seg_norm_relu_backward(x.data_ptr(), ab.data_ptr(), None, gv.data_ptr(), n, c, hw, _ptr(gx),
                                                None, None, None, 0, _lib.stream_ptr()))
        return gx, None, None
    dg, db = torch.zeros(c, dtype=torch.float32, device=x.device), torch.zeros(c, dtype=torch.float32, device=x.device)
    ws = _ws(L.cae_seg_norm_workspace(n, c), x.device)
    _lib.check(L.cae_seg_norm_relu_backward(x.data_ptr(), ab.data_ptr(), _f32(gamma).data_ptr(), gv.data_ptr(), n, c, hw,
                                            _ptr(gx), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                            _lib.stream_ptr()))
    return gx, dg, db


def channel_sums(g: torch.Tensor) -> torch.Tensor:
    """cae_seg_channel_sums: (n, c, ...) -> (c,)"""
    g = _f32(g)
    n, c = g.shape[:2]
    out = torch.zeros(c, dtype=torch.float32, device=g.device)
    if n:
        L = _lib.lib()
        ws = _ws(L.cae_seg_channel_sums_workspace(n, c), g.device)
        _lib.check(L.cae_seg_channel_sums(g.data_ptr(), n, c, g[0, 0].numel(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                          _lib.stream_ptr()))
    return out


# ---- the head's autograd function ----------------------------------------------------------------------------------
WEIGHT_EXP = 15  # the data gradient reads its weight scaled to max|w| in [2^14, 2^15), below the f16 maximum 65504


def grad_scale(m: float) -> float:
    """s = 2^-floor(log2 m): s m lies in [1, 2)"""
    return math.ldexp(1.0, -(math.frexp(m)[1] - 1))


class _HeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, n_brg, *tensors):
        brg, params = list(tensors[:n_brg]), tensors[n_brg:]
        logits, saved = model._forward_taps(x, brg)
        ctx.model, ctx.saved, ctx.n_brg, ctx.n_params = model, saved, n_brg, len(params)
        ctx.x, ctx.brg = x, brg
        return logits

    @staticmethod
    def backward(ctx, g_logits):
        model, saved = ctx.model, ctx.saved
        grads = model._backward(ctx.x, ctx.brg, saved, g_logits)
        return (None, None, None) + (None,) * ctx.n_brg + tuple(grads)


class JNetTrain(JNet):
    """``segmenters.JNet`` with a backward pass: same constructor, same state-dict keys, order and shapes."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._weight_ticket = None
        self._bwd_flags: List[torch.Tensor] = []
        self.last_grad_stats: Optional[Dict] = None  # per-stage max|s g| of the latest backward when record_grad_stats
        self.record_grad_stats = False

    # ---- weights: refreshed on the device ----------------------------------------------------------------------------
    def _sync(self):
        ws = self._weight_list()
        if self._handle is None or not all(w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() for w in ws):
            self._uploaded = None
            return super()._sync()
        # (always: the fused optimiser step writes the parameters without touching their version counters)
        ptrs = (ctypes.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        L = _lib.lib()
        _lib.check(L.cae_seg_set_weights(self._handle.ptr, ptrs, len(ws), _lib.stream_ptr()))
        self._weight_ticket = L.cae_seg_last_ticket()
        return self._handle

    def _check_weights(self):
        """after the stream work has completed: did the latest device refresh see a weight outside the f16 range?"""
        ticket, self._weight_ticket = self._weight_ticket, None
        if ticket is None:
            return
        try:
            _lib.check(_lib.lib().cae_seg_range_check(self._handle.ptr, ticket))
        except FloatingPointError:
            raise ValueError('segmentation head: a weight, gamma or beta entry is outside the f16 range (|v| <= 65504, '
                             'finite); the head has no fp32 path') from None

    # ---- call surface ------------------------------------------------------------------------------------------------
    def _check(self, x, fx_brg):
        if torch.is_grad_enabled() and (x.requires_grad or any(b.requires_grad for b in (fx_brg or []))):
            raise NotImplementedError(JOINT)
        was = self.training
        self.training = False  # (GroupNorm keeps no running statistics: both modes compute the same)
        try:
            with torch.no_grad():  # the shape checks of the inference head
                return super()._check(x, fx_brg)
        finally:
            self.training = was

    def forward(self, x: torch.Tensor, fx_brg=None, taps: bool = False):
        if torch.is_grad_enabled() and (x.requires_grad or any(b.requires_grad for b in (fx_brg or []))):
            raise NotImplementedError(JOINT)
        recording = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if not recording or taps:
            with torch.no_grad():
                out = super().forward(x, fx_brg, taps=taps)
            self._check_weights()
            return out
        x, brg = self._stage(x, self._check(x, fx_brg))
        if self.force_torch:
            return self._forward_torch(x, brg), None
        params = self._weight_list()
        if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params):
            raise ValueError('training the head needs its parameters as contiguous fp32 tensors on the device (.cuda())')
        return _HeadFunction.apply(self, x, len(brg), *brg, *params), None

    def _pairs(self, t: torch.Tensor, norm) -> torch.Tensor:
        """(a, b) of relu(GroupNorm_C(t)) in the taps' layout, from two-pass double statistics of the planes: a = gamma
        rstd, b = fma(-mean, a, beta); norm None (no normalisation): (1, 0).  Padding channels (0, 0)."""
        n, c = t.shape[:2]
        ab = torch.zeros((n, (c + 7) // 8 * 8, 2), dtype=torch.float32, device=t.device)
        if norm is None:
            ab[:, :c, 0] = 1.0
            return ab
        mean = t.mean(dim=(2, 3), dtype=torch.float64)  # (the reductions convert as they read: no double copy of t)
        var = (t - mean.float()[:, :, None, None]).square_().mean(dim=(2, 3), dtype=torch.float64)
        a = (norm.weight.detach().double()[None] * torch.rsqrt(var + segmenters.EPS)).float()
        ab[:, :c, 0] = a
        ab[:, :c, 1] = (norm.bias.detach().double()[None] - mean * a.double()).float()
        return ab

    def _forward_taps(self, x, brg):
        """The training forward, stage by stage over ``cae_seg_conv2d`` (the forward kernel on freshly packed weights) with
        every weight scaled to max|w| in [2^14, 2^15) before the split and the output scaled back: the fused
        ``cae_seg_forward`` packs the weights as they are, and weights below 2^-3 (every canonical layer) then keep 2^-25
        absolute instead of 2^-22 relative, which the gradients of the canonical head do not tolerate.  A
        stage over two concatenated sources is the sum of two convolutions.  -> (logits, taps as JNet._taps lays them
        out); asynchronous, the range word joins the backward's."""
        plan, bn = self.stage_plan(), self._batch_norm
        flag = new_flag(x.device)
        one = torch.ones((), dtype=torch.float32, device=x.device)
        raw: List[torch.Tensor] = []
        ab: List[Optional[torch.Tensor]] = []
        bab = [self._pairs(b, self.bridges_projection[i]._bn1 if bn else None) for i, b in enumerate(brg)]
        for st in plan:
            w, bias = st['weight'].detach(), st['bias']
            if st['up']:  # four pointwise matrices, row 4 co + 2 dy + dx, then the pixel shuffle
                cin, cout = w.shape[:2]
                w = w.permute(1, 2, 3, 0).reshape(4 * cout, cin, 1, 1)
                bias = None if bias is None else bias.detach().repeat_interleave(4)
            elif bias is not None:
                bias = bias.detach()
            sw = torch.ldexp(one, WEIGHT_EXP - torch.frexp(w.abs().max())[1])
            out, c0 = None, 0
            for src in st['srcs']:
                if src[0] == 'latent':
                    t, t_ab = x, None
                elif src[0] == 'bridge':
                    t, t_ab = brg[src[1]], bab[src[1]]
                else:
                    t, t_ab = raw[src[1]], (ab[src[1]] if src[2] else None)
                part = conv2d(t, (w[:, c0:c0 + t.size(1)] * sw).contiguous(), None if (bias is None or c0) else bias * sw,
                              flag, t_ab)
                out = part if out is None else out.add_(part)
                c0 += t.size(1)
            out.mul_(1.0 / sw)
            raw.append(F.pixel_shuffle(out, 2) if st['up'] else out)
            ab.append(self._pairs(raw[-1], st['norm']) if st['has_ab'] else None)
        self._bwd_flags.append(flag)
        # (a copy: the function's output must not be the tensor its own context keeps, or every step's taps wait for the
        # cycle collector)
        return raw[-1].clone(), dict(plan=plan, raw=raw, ab=ab, bridge_ab=bab, ticket=None)

    def _backward(self, x, brg, saved, g_logits) -> List[Optional[torch.Tensor]]:
        plan, raw, ab, bab = saved['plan'], saved['raw'], saved['ab'], saved['bridge_ab']
        params = self._weight_list()
        g = g_logits.detach().to(torch.float32).contiguous()
        m = float(g.abs().max()) if g.numel() else 0.0  # the step's one synchronisation
        self._check_weights()
        if saved['ticket'] is not None:
            _lib.check(_lib.lib().cae_seg_range_check(self._handle.ptr, saved['ticket']))  # FloatingPointError
        if not math.isfinite(m):
            raise FloatingPointError('segmentation head: the gradient of the logits is not finite')
        if m == 0.0:
            return [torch.zeros_like(p) if p.requires_grad else None for p in params]
        s = grad_scale(m)
        flag = new_flag(g.device)
        bn = self._batch_norm
        out: Dict[int, tuple] = {}  # id(parameter) -> (scaled gradient, its scale as a device scalar)
        graw: Dict[int, tuple] = {len(plan) - 1: (g * s, torch.full((), s, dtype=torch.float32, device=g.device))}
        stats = {} if self.record_grad_stats else None
        one = torch.ones((), dtype=torch.float32, device=g.device)

        def source(src):
            """-> (tensor, ab or None, wants a data gradient)"""
            if src[0] == 'latent':
                return x, None, False
            if src[0] == 'bridge':
                return brg[src[1]], bab[src[1]], bn
            return raw[src[1]], (ab[src[1]] if src[2] else None), True

        for k in reversed(range(len(plan))):
            st, (G, cum) = plan[k], graw.pop(k)
            # every stage's gradient is brought back to max|G| in [1, 2) by an exact power of two, on the device
            mx = G.abs().max()
            sk = torch.ldexp(one, 1 - torch.frexp(mx)[1])
            G, cum = G * sk, cum * sk
            if stats is not None:
                stats[st['name']] = mx / (cum / sk) * s  # max|s g| of this stage under the step's one scale
            w = st['weight']
            srcs = [source(sr) for sr in st['srcs']]
            if st['bias'] is not None:
                out[id(st['bias'])] = (channel_sums(G), cum)
            if st['up']:
                G = F.pixel_unshuffle(G, 2)  # channel 4 co + 2 dy + dx
                cin, cout = w.shape[:2]
                out[id(w)] = (wgrad(G, [srcs[0][:2]], 1, flag).reshape(cout, 2, 2, cin).permute(3, 0, 1, 2).contiguous(), cum)
                wd = w.detach().reshape(cin, 4 * cout, 1, 1)
            else:
                out[id(w)] = (wgrad(G, [sr[:2] for sr in srcs], st['ks'], flag), cum)
                wd = w.detach().flip(2, 3).transpose(0, 1).contiguous()
            if not any(sr[2] for sr in srcs):
                continue
            # the data gradient's weight is brought to max|w| in [2^14, 2^15) like G to [1, 2): at |w| < 2^-3 the low half of
            # the f16 split is subnormal and keeps 2^-25 absolute, not 2^-22 relative (canonical weights are near 0.01)
            sw = torch.ldexp(one, WEIGHT_EXP - torch.frexp(wd.abs().max())[1])
            gv, c0, cum = conv2d(G, wd * sw, None, flag), 0, cum * sw
            for sr, (t, t_ab, want) in zip(st['srcs'], srcs):
                piece = gv if len(srcs) == 1 else gv[:, c0:c0 + t.size(1)].contiguous()
                c0 += t.size(1)
                if not want:
                    continue
                if sr[0] == 'bridge':  # the projection's _bn1 on a codec tensor: gamma and beta only
                    bn1 = self.bridges_projection[sr[1]]._bn1
                    _, dg, db = norm_relu_backward(t, t_ab, bn1.weight.detach(), piece, False)
                    out[id(bn1.weight)], out[id(bn1.bias)] = (dg, cum), (db, cum)
                elif not sr[2]:
                    graw[sr[1]] = (piece, cum)
                else:
                    norm = plan[sr[1]]['norm']
                    gx, dg, db = norm_relu_backward(t, t_ab, None if norm is None else norm.weight.detach(), piece)
                    graw[sr[1]] = (gx, cum)
                    if norm is not None:
                        out[id(norm.weight)], out[id(norm.bias)] = (dg, cum), (db, cum)
        live = [out[id(p)] for p in params if id(p) in out]
        torch._foreach_mul_([t for t, _ in live], [1.0 / c for _, c in live])
        self._bwd_flags.append(flag)
        if stats is not None:
            self.last_grad_stats = dict(scale=s, max_g_logits=m, stages={k: float(v) for k, v in stats.items()})
        return [out[id(p)][0] if p.requires_grad and id(p) in out else None for p in params]

    def backward_flags(self) -> Optional[torch.Tensor]:
        """the overflow words of the backward passes since the last check, as one device tensor (or None)"""
        flags, self._bwd_flags = self._bwd_flags, []
        return torch.cat(flags) if flags else None

    def check_backward(self):
        """FloatingPointError if a backward pass since the last check staged a value outside the f16 range: its gradients
        are invalid (one device read)."""
        flags = self.backward_flags()
        if flags is not None and bool(flags.any()):
            raise FloatingPointError('segmentation head backward: a staged gradient or activation left the valid range of '
                                     'the f16x3 kernels (finite, |v| <= 65504); the gradients of that step are invalid')


# ---- loader, forward function, losses, optimiser, step ---------------------------------------------------------------
def setup_modules(segment_model_type='JNet', **kwargs):
    if segment_model_type != 'JNet':
        raise NotImplementedError(f'only the JNet head is trainable, got {segment_model_type!r}')
    return JNetTrain(**kwargs)


def segmenter_from_state_dict(checkpoint, gpu=False, train=True):
    """The reference's loader (``_segmenters.py:347``) -> ``JNetTrain``; ``gpu`` is accepted for signature compatibility."""
    return segmenters.load_segmenter(checkpoint, setup_modules, train, trainable=True)


def setup_forward_func(enabled_modules: Sequence[str] = ('encoder', 'fact_ent', 'decoder', 'seg_model'),
                       trainable_modules: Sequence[str] = ('seg_model',)):
    """decorate_trainable_modules of the reference for head training: the codec modules run under ``torch.no_grad()``,
    the head under grad.  Returns the same dict as ``criteria.setup_forward_func``."""
    enabled, trainable = set(enabled_modules), set(trainable_modules)
    unknown = enabled - {'encoder', 'fact_ent', 'decoder', 'seg_model'}
    if unknown:
        raise NotImplementedError(f'modules outside the compression path are not built: {sorted(unknown)}')
    if trainable - {'seg_model'}:
        raise NotImplementedError(JOINT)

    def forward_func(x, model) -> Dict:
        with torch.no_grad():
            y = model['encoder'](x) if 'encoder' in enabled else x
            y_q, p_y = model['fact_ent'](y) if 'fact_ent' in enabled else (y, None)
            x_r, fx_brg = model['decoder'](y_q) if 'decoder' in enabled else (y_q, None)
        s_pred = s_aux_pred = None
        if 'seg_model' in enabled:
            with torch.set_grad_enabled(torch.is_grad_enabled() and 'seg_model' in trainable):
                s_pred, s_aux_pred = model['seg_model'](y_q, fx_brg=fx_brg)
        return dict(x_r=x_r, fx_brg=fx_brg, y=y, y_q=y_q, p_y=p_y, t_pred=None, t_aux_pred=None, s_pred=s_pred,
                    s_aux_pred=s_aux_pred)

    return forward_func


class SegLoss:
    """``criteria/_classification.py``: 'BCELoss' (BCEWithLogits, mean), 'CELoss' (CrossEntropy, mean), 'WeightedBCELoss'
    (t[:, :1] weights the elementwise BCEWithLogits of t[:, 1:], then the mean).  Torch ops on the device."""
    TYPES = ('BCELoss', 'WeightedBCELoss', 'CELoss')

    def __init__(self, class_loss_type: str = 'BCELoss', **kwargs):
        if class_loss_type not in self.TYPES:
            raise NotImplementedError(f'class_loss_type must be one of {self.TYPES} (the *WithAux losses need an aux '
                                      f'prediction the head does not return), got {class_loss_type!r}')
        self.class_loss_type = class_loss_type

    def __call__(self, pred, t, **kwargs):
        t = t.to(pred.device)
        if self.class_loss_type == 'CELoss':
            loss = F.cross_entropy(pred, t)
        elif self.class_loss_type == 'BCELoss':
            loss = F.binary_cross_entropy_with_logits(pred, t)
        else:
            loss = torch.mean(t[:, :1] * F.binary_cross_entropy_with_logits(pred, t[:, 1:], reduction='none'))
        return dict(class_error=loss, aux_class_error=0)


def setup_optim(model, learning_rate: float = 1e-4, weight_decay: float = 0.0, algo=torch.optim.Adam
                ) -> Dict[str, torch.optim.Optimizer]:
    """One optimiser over the head's parameters (``model``: the head, or a module dict with 'seg_model')."""
    head = model['seg_model'] if isinstance(model, (dict, nn.ModuleDict)) else model
    return {'seg_model': algo([dict(params=list(head.parameters()), lr=learning_rate, weight_decay=weight_decay)])}


def train_step(x, t, model, criterion, optimizers, forward_func=None):
    """One iteration of head training: forward, loss, backward, clip at norm 1.0 and step.  ``model``: a module dict
    with 'seg_model' (and the codec modules ``forward_func`` enables).  -> loss_dict (detached scalars)"""
    from .train import fused_clip_adam
    forward_func = forward_func or setup_forward_func()
    output = forward_func(x, model)
    loss_dict = criterion(pred=output['s_pred'], t=t)
    loss_dict['class_error'].backward()
    head = model['seg_model']
    if isinstance(head, JNetTrain):
        head.check_backward()
    if not fused_clip_adam(optimizers, max_norm=1.0):
        for opt in optimizers.values():
            nn.utils.clip_grad_norm_(opt.param_groups[0]['params'], max_norm=1.0)
            opt.step()
            opt.zero_grad()
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in loss_dict.items()}
