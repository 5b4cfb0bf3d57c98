"""Training path on the HIP kernels (BASELINE config 5).

What the reference's training step does (``src/train_cae_ms.py:189-262``) and where it lives here:

* ``forward_func`` (``models/tasks/_taskutils.py:95-108``): encoder -> fact_ent (train mode: additive U(-1/2, 1/2)
  noise) -> decoder.  ``Analyzer.forward`` / ``Synthesizer.forward`` switch to the differentiable track functions of
  this module whenever autograd is recording: bf16 convolutions with fp32 accumulation
  (``cae_t_conv_forward_act`` / ``cae_t_deconv_forward_act``), fp32 GDN / IGDN (``cae_t_gdn_forward_save``), and
  hand-written backward kernels (data gradients, weight gradients, GDN gradient) instead of ATen / cuDNN autograd.
* ``GeneralLoss`` (``models/criteria/_lossutils.py:54-109``): ``criteria.GeneralLoss`` (scalar reductions, torch ops).
* compressai's ``NonNegativeParametrizer`` / ``LowerBound`` gradient rule of the GDN parameters: the kernels
  differentiate with respect to the EFFECTIVE beta / gamma, the reparametrisation stays a torch autograd graph
  (``modules.NonNegativeParametrizer``), so the rule (pass where ``p >= bound`` or ``grad < 0``) is applied exactly
  once, on parameter-sized tensors.
* ``setup_optim`` (``train_cae_ms.py:529-655``): one optimiser per trainable module, the ``quantiles`` of the entropy
  model in a separate ``<module>_aux`` optimiser (:592-596); ``train_step`` = :209-230 (loss.backward, aux_loss.backward,
  per-optimiser clip_grad_norm_(1.0), step, zero_grad).
* ``nn.DataParallel``'s gradient reduction (``_autoencoders.py:517``): ``GradReducer``, bucketed all-reduce over
  ``torch.distributed`` (RCCL over xGMI on GPUs, gloo on CPU), one process per GPU.

Variants covered: ``act_layer_type in (None, 'GDN', 'LeakyReLU', 'ReLU')`` units (the last two with their stride-1
pre-convolutions) on the fused track functions, and residual units (``use_residual=True``) composed per operation from
the same kernels (``_composed_track``), as are units with batch norm in training mode (batch statistics, running
statistics updated as ``nn.BatchNorm2d`` does), grouped layers (dense kernels on the block-diagonal embedding of the
grouped weight) and ``Dropout2d``.  Multiscale colour layers (``multiscale_analysis``, _autoencoders.py:417-452) train
on both forms: inside ``SynthesisFn`` (their data gradient summed with the next unit's before the level's IGDN / activation
backward) and as ``_ColourFn`` behind the units of a composed track; ``criteria.DistMSEPyramidLoss`` scores them.

The host layer, top down: ONE launch wrapper per ``cae_t_*`` entry point, its only call site (tensors and the few real
choices in; every integer derived from tensor shapes, a convolution's channel counts and kernel size from the packed weight
of ``_pack``; outputs allocated and returned); the steps, each written once (``_conv_s1_forward`` / ``_conv_s1_backward``,
``_conv_s2_backward``, ``_layer_forward``, ``_hand_down``); the autograd functions of the fused and the composed tracks as
drivers over the steps.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import os

import torch
import torch.nn as nn

from . import _lib

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _pad32(c: int) -> int:
    return (int(c) + 31) // 32 * 32


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _L():
    return _lib.lib()


def _st():
    return _lib.stream_ptr()


def _new(ref: torch.Tensor, shape, dtype) -> torch.Tensor:
    return torch.empty(shape, dtype=dtype, device=ref.device)


class LayerSpec:
    """Static description of one unit for the track functions."""

    def __init__(self, cin: int, cout: int, ks: int, has_bias: bool, has_gdn: bool, act: int = 0, has_pre: bool = False):
        self.cin, self.cout, self.ks = int(cin), int(cout), int(ks)
        self.cin_p, self.cout_p = _pad32(cin), _pad32(cout)
        self.has_bias, self.has_gdn = bool(has_bias), bool(has_gdn)
        # LeakyReLU (1) / ReLU (2) units: activation after the strided layer, and (has_pre) a stride-1 convolution
        # cin -> cin + the same activation in front of it (_autoencoders.py:62-76, :187-202)
        self.act, self.has_pre = int(act), bool(has_pre)

    @property
    def n_tensors(self) -> int:
        return (1 + int(self.has_bias)) * (1 + int(self.has_pre)) + 2 * int(self.has_gdn)


class ColourSpec:
    """One multiscale colour layer: Conv2d(cin -> cout, ks, stride 1, reflect padding ks//2) (_autoencoders.py:417-428)."""

    def __init__(self, cin: int, cout: int, ks: int, has_bias: bool):
        self.cin, self.cout, self.ks, self.has_bias = int(cin), int(cout), int(ks), bool(has_bias)
        self.cin_p = _pad32(cin)
        self.K = self.ks * self.ks * self.cout  # GEMM columns (tap, channel) of the edge form
        self.kp = _pad32(self.K)

    @property
    def n_tensors(self) -> int:
        return 1 + int(self.has_bias)


def _split_params(specs: Sequence[LayerSpec], tensors: Sequence[torch.Tensor]):
    """-> per layer (w, b, beta, gamma, pre_w, pre_b); flat order: [pre_w, pre_b?]? w, b?, [beta, gamma]?"""
    out, it = [], iter(tensors)
    for s in specs:
        pw = next(it) if s.has_pre else None
        pb = next(it) if s.has_pre and s.has_bias else None
        w = next(it)
        b = next(it) if s.has_bias else None
        beta, gamma = (next(it), next(it)) if s.has_gdn else (None, None)
        out.append((w, b, beta, gamma, pw, pb))
    return out


def _flat_grads(specs, per_layer):
    """per_layer[i] = [g_w, g_b, g_beta, g_gamma, g_pre_w, g_pre_b] -> the flat order of _split_params"""
    out: List[Optional[torch.Tensor]] = []
    for s, (g_w, g_b, g_beta, g_gamma, g_pw, g_pb) in zip(specs, per_layer):
        if s.has_pre:
            out.append(g_pw)
            if s.has_bias:
                out.append(g_pb)
        out.append(g_w)
        if s.has_bias:
            out.append(g_b)
        if s.has_gdn:
            out.extend([g_beta, g_gamma])
    return out


def _split_colour(colour, tensors):
    """flat colour tensors -> per level (w, b | None)"""
    out, k = [], 0
    for cs in colour:
        out.append((tensors[k], tensors[k + 1] if cs.has_bias else None))
        k += cs.n_tensors
    return out


def _detached(layers):
    return [tuple(t.detach() if t is not None else None for t in l) for l in layers]


# ---- weights as the kernels read them ---------------------------------------------------------------------------------

def _pack(weight: torch.Tensor, contract_dim: int, ks: int) -> torch.Tensor:
    """fp32 (d0, d1, k, k) -> bf16 MFMA B fragments on the device (cae_t_pack_weights), shaped [k*k][kc_p][nc_p] (kc the
    contracted, nc the produced channels, padded to 32: the element count; the order inside is the kernels' own).  The
    launch wrappers read the kernel size and both channel counts of a convolution from this shape."""
    d0, d1 = weight.shape[0], weight.shape[1]
    kc, nc = (d0, d1) if contract_dim == 0 else (d1, d0)
    out = torch.empty((ks * ks, _pad32(kc), _pad32(nc)), dtype=BF16, device=weight.device)
    if _L().cae_t_packed_bytes(kc, nc, ks) != 2 * out.numel():
        raise ValueError(f'packed size of a ({d0}, {d1}, {ks}, {ks}) weight is not that of {tuple(out.shape)} bf16')
    w = weight.detach().float().contiguous()
    _lib.check(_L().cae_t_pack_weights(w.data_ptr(), d0, d1, ks, contract_dim, out.data_ptr(), _st()))
    return out


def _packed_dims(wp: torch.Tensor, contracted: int):
    """-> (ks, produced padded channels) of a packed weight that must contract over `contracted` padded channels"""
    kk, kc_p, nc_p = wp.shape
    ks = int(round(kk ** 0.5))
    if kc_p != contracted or ks * ks != kk:
        raise ValueError(f'packed weight {tuple(wp.shape)} does not contract over {contracted} channels')
    return ks, nc_p


def _bias_p(b: Optional[torch.Tensor], cp: int, dev) -> Optional[torch.Tensor]:
    if b is None:
        return None
    out = torch.zeros(cp, dtype=F32, device=dev)
    out[:b.numel()] = b.detach().float()
    return out


def _pack_bias(w: torch.Tensor, b: Optional[torch.Tensor], contract_dim: int, ks: int):
    """-> (packed weight, bias padded to its produced channels | None)"""
    wp = _pack(w, contract_dim, ks)
    return wp, _bias_p(b, wp.shape[2], w.device)


def _edge_ok(spec: 'LayerSpec', c_img: int) -> bool:
    """the 3-channel edge of a track as a pointwise GEMM over K = (tap, channel) <= 32 (cae_t_im2col_s2 / cae_t_col2im_s2):
    no stride-1 pre-convolution at that edge, k^2 * channels fits one 32-deep chunk; CAE_EDGE_GEMM=0 keeps the padded form"""
    return (not spec.has_pre and spec.ks * spec.ks * c_img <= 32 and os.environ.get('CAE_EDGE_GEMM', '1') != '0')


def _colour_edge(cs: ColourSpec) -> bool:
    """the colour layer as a pointwise GEMM over K = (tap, channel) <= 96 (cae_t_col2im_s1r / cae_t_im2col_s1r); else, or with
    CAE_EDGE_GEMM=0, the padded stride-1 form on the convolution kernels (cae_t_corr_s1 / cae_t_wgrad_s1)"""
    return cs.cout <= 3 and cs.kp <= 96 and os.environ.get('CAE_EDGE_GEMM', '1') != '0'


def _pack_1x1(m: torch.Tensor, rows: int, cols: int, again_at: Optional[int] = None) -> torch.Tensor:
    """the matrix m (produced, contracted), zero-padded to (rows, cols), as the packed weight of a 1 x 1 GEMM; again_at: a
    second copy of m from that column on (the (hi, lo) halves of the colour layer's gradient columns)"""
    w1 = torch.zeros((rows, cols, 1, 1), dtype=F32, device=m.device)
    w1[:m.shape[0], :m.shape[1], 0, 0] = m
    if again_at is not None:
        w1[:m.shape[0], again_at:again_at + m.shape[1], 0, 0] = m
    return _pack(w1, 1, 1)


def _first_layer_1x1(wt: torch.Tensor, s: LayerSpec) -> torch.Tensor:
    """analysis edge: (cout, cin, k, k) contracting over the im2col columns (tap, ci), 27 of 32"""
    return _pack_1x1(wt.detach().float().permute(0, 2, 3, 1).reshape(s.cout, -1), s.cout, 32)


def _last_layer_1x1(wt: torch.Tensor, s: LayerSpec, dgrad: bool) -> torch.Tensor:
    """synthesis edge: (cin, cout, k, k) producing the col2im columns j = (tap, co) from the channels, or (dgrad) the
    channels' gradient from the columns of the output gradient's im2col"""
    K = s.ks * s.ks * s.cout
    if dgrad:
        return _pack_1x1(wt.detach().float().permute(0, 2, 3, 1).reshape(s.cin, K), s.cin, 32)
    return _pack_1x1(wt.detach().float().permute(2, 3, 1, 0).reshape(K, s.cin), 32, s.cin)


def _colour_1x1(wt: torch.Tensor, cs: ColourSpec, dgrad: bool) -> torch.Tensor:
    """colour edge form: (cout, cin, k, k) producing the kp columns j = (tap, co), or (dgrad) the channels' gradient from
    the 2 kp (hi, lo) gradient columns, the weights repeated over both halves"""
    if dgrad:
        return _pack_1x1(wt.detach().float().permute(1, 2, 3, 0).reshape(cs.cin, cs.K), cs.cin, 2 * cs.kp, again_at=cs.kp)
    return _pack_1x1(wt.detach().float().permute(2, 3, 0, 1).reshape(cs.K, cs.cin), cs.kp, cs.cin)


# ---- launch wrappers: one per cae_t_* entry point, every integer from tensor shapes -----------------------------------

def _from_nchw(x: torch.Tensor, cp: int, want16=True, want32=False):
    n, c, h, w = x.shape
    x = x.detach().float().contiguous()
    o16 = _new(x, (n, h, w, cp), BF16) if want16 else None
    o32 = _new(x, (n, h, w, cp), F32) if want32 else None
    _lib.check(_L().cae_t_from_nchw(x.data_ptr(), n, c, h, w, cp, _ptr(o16), _ptr(o32), _st()))
    return o16, o32


def _to_nchw(t32: torch.Tensor, c: int) -> torch.Tensor:
    n, h, w, cp = t32.shape
    out = _new(t32, (n, c, h, w), F32)
    _lib.check(_L().cae_t_to_nchw(t32.data_ptr(), n, c, h, w, cp, out.data_ptr(), _st()))
    return out


def _colsum(g16, c):
    n, h, w, cp = g16.shape
    gb = _new(g16, cp, F32)
    _lib.check(_L().cae_t_colsum(g16.data_ptr(), n * h * w, cp, gb.data_ptr(), _st()))
    return gb[:c].clone()


def _act_backward(g16, gext32, pad, y16, act):
    """gradient through LeakyReLU / ReLU: g * (y > 0 ? 1 : slope), y = the activation's output; g bf16, or the fp32
    extended-domain gradient (folded in place first) -> bf16"""
    n, h, w, cp = y16.shape
    out = torch.empty_like(y16)
    _lib.check(_L().cae_t_act_backward(_ptr(g16), _ptr(gext32), pad, y16.data_ptr(), n, h, w, cp, act, out.data_ptr(), _st()))
    return out


def _fold_to_bf16(t32: torch.Tensor, pad: int = 0) -> torch.Tensor:
    """fp32 [n][h + 2 pad][w + 2 pad][cp], the reflect border folded onto the interior (in place) -> bf16 [n][h][w][cp];
    pad 0: the plain rounding"""
    n, hp, wp, cp = t32.shape
    h, w = hp - 2 * pad, wp - 2 * pad
    out = torch.empty_like(t32, dtype=BF16) if pad == 0 else _new(t32, (n, h, w, cp), BF16)
    _lib.check(_L().cae_t_fold_to_bf16(t32.data_ptr(), n, h, w, pad, cp, out.data_ptr(), _st()))
    return out


def _fold_acc(gext32: torch.Tensor, pad: int, acc32: torch.Tensor) -> None:
    """acc32 += the reflect fold of gext32 (extended by pad)"""
    n, h, w, cp = acc32.shape
    assert gext32.shape == (n, h + 2 * pad, w + 2 * pad, cp)
    _lib.check(_L().cae_t_fold_acc(gext32.data_ptr(), n, h, w, pad, cp, acc32.data_ptr(), _st()))


def _two_outputs(ref, shape, want32, want16):
    return (_new(ref, shape, F32) if want32 else None), (_new(ref, shape, BF16) if want16 else None)


def _conv_fwd(a16, wp, bias_p, act, want32):
    """reflect convolution, stride 2 (+ bias): -> (fp32 output, None) or (None, bf16 output behind the activation)"""
    n, h, w, cin_p = a16.shape
    ks, cout_p = _packed_dims(wp, cin_p)
    z32, z16 = _two_outputs(a16, (n, (h + 1) // 2, (w + 1) // 2, cout_p), want32, not want32)
    _lib.check(_L().cae_t_conv_forward_act(a16.data_ptr(), n, h, w, cin_p, wp.data_ptr(), ks, _ptr(z32), _ptr(z16), cout_p,
                                           _ptr(bias_p), act, _st()))
    return z32, z16


def _deconv_fwd(a16, wp, bias_p, act, want32):
    """transposed convolution, stride 2 (+ bias): outputs as _conv_fwd"""
    n, h, w, cin_p = a16.shape
    ks, cout_p = _packed_dims(wp, cin_p)
    z32, z16 = _two_outputs(a16, (n, 2 * h, 2 * w, cout_p), want32, not want32)
    _lib.check(_L().cae_t_deconv_forward_act(a16.data_ptr(), n, h, w, cin_p, wp.data_ptr(), ks, _ptr(z32), _ptr(z16), cout_p,
                                             _ptr(bias_p), act, _st()))
    return z32, z16


def _pointwise(a16, wp, bias_p, act, want32):
    """1 x 1 GEMM over the channels (+ bias): outputs as _conv_fwd"""
    n, h, w, cp = a16.shape
    _, cn = _packed_dims(wp, cp)
    o32, o16 = _two_outputs(a16, (n, h, w, cn), want32, not want32)
    _lib.check(_L().cae_t_pointwise(a16.data_ptr(), n, h, w, cp, wp.data_ptr(), _ptr(o32), _ptr(o16), cn, _ptr(bias_p), act,
                                    _st()))
    return o32, o16


def _pointwise_acc(a16, wp, acc32) -> None:
    """acc32 += the 1 x 1 GEMM of a16"""
    n, h, w, cp = a16.shape
    _, cn = _packed_dims(wp, cp)
    assert acc32.shape == (n, h, w, cn)
    _lib.check(_L().cae_t_pointwise_acc(a16.data_ptr(), n, h, w, cp, wp.data_ptr(), acc32.data_ptr(), cn, _st()))


def _corr_s1(a16, wp, mode, bias_p=None, act=0, want32=True, want16=False):
    """stride-1 correlation.  mode 0: reflect convolution, 2: transposed convolution (padding k//2), 3: its data gradient,
    1: the reflect convolution's data gradient on the EXTENDED domain (k//2 more on every side, to be folded).
    -> (fp32 output | None, bf16 output behind the activation | None)"""
    n, h, w, cp = a16.shape
    ks, cn = _packed_dims(wp, cp)
    ext = ks // 2 if mode == 1 else 0
    o32, o16 = _two_outputs(a16, (n, h + 2 * ext, w + 2 * ext, cn), want32, want16)
    _lib.check(_L().cae_t_corr_s1(a16.data_ptr(), n, h, w, cp, wp.data_ptr(), ks, mode, _ptr(o32), _ptr(o16), cn, _ptr(bias_p),
                                  act, _st()))
    return o32, o16


def _wgrad(fine16, coarse16, ks, reflect):
    """weight gradient of a stride-2 layer from its fine-resolution and coarse-resolution operands -> [k*k][c fine][c coarse];
    reflect 1: the convolution (input fine, output gradient coarse), 0: the transposed one (output gradient fine)"""
    n, h, w, cf = fine16.shape
    _, oh, ow, cc = coarse16.shape
    assert (oh, ow) == ((h + 1) // 2, (w + 1) // 2) and coarse16.shape[0] == n
    gw = _new(fine16, (ks * ks, cf, cc), F32)
    _lib.check(_L().cae_t_wgrad(fine16.data_ptr(), n, h, w, cf, coarse16.data_ptr(), oh, ow, cc, ks, reflect, gw.data_ptr(), _st()))
    return gw


def _wgrad_s1(a16, b16, ks, reflect):
    """weight gradient of a stride-1 layer -> [k*k][ca][cb]; reflect 1: (input, output gradient) of the reflect convolution,
    0: (output gradient, input) of the transposed one"""
    n, h, w, ca = a16.shape
    assert b16.shape[:3] == (n, h, w)
    gw = _new(a16, (ks * ks, ca, b16.shape[3]), F32)
    _lib.check(_L().cae_t_wgrad_s1(a16.data_ptr(), n, h, w, ca, b16.data_ptr(), b16.shape[3], ks, reflect, gw.data_ptr(), _st()))
    return gw


def _wgrad_pointwise(a16, g16):
    """weight gradient of a 1 x 1 GEMM -> [1][ca][cg]"""
    n, h, w, ca = a16.shape
    assert g16.shape[:3] == (n, h, w)
    gw = _new(a16, (1, ca, g16.shape[3]), F32)
    _lib.check(_L().cae_t_wgrad_pointwise(a16.data_ptr(), g16.data_ptr(), n, h, w, ca, g16.shape[3], gw.data_ptr(), _st()))
    return gw


def _conv_dgrad_ext(g16, wp, hw):
    """data gradient of the stride-2 reflect convolution of an h x w input, on the extended domain (fp32, to be folded)"""
    n, oh, ow, cout_p = g16.shape
    (h, w), (ks, cin_p) = hw, _packed_dims(wp, cout_p)
    assert (oh, ow) == ((h + 1) // 2, (w + 1) // 2)
    gext = _new(g16, (n, h + 2 * (ks // 2), w + 2 * (ks // 2), cin_p), F32)
    _lib.check(_L().cae_t_conv_dgrad_ext(g16.data_ptr(), n, oh, ow, cout_p, wp.data_ptr(), ks, h, w, gext.data_ptr(), cin_p, _st()))
    return gext


def _deconv_dgrad(g16, wp, want32):
    """data gradient of the stride-2 transposed convolution -> (fp32 | None, bf16 | None)"""
    n, h2, w2, cout_p = g16.shape
    ks, cin_p = _packed_dims(wp, cout_p)
    gx32, gx16 = _two_outputs(g16, (n, h2 // 2, w2 // 2, cin_p), want32, not want32)
    _lib.check(_L().cae_t_deconv_dgrad(g16.data_ptr(), n, h2 // 2, w2 // 2, cout_p, wp.data_ptr(), ks, _ptr(gx32), _ptr(gx16),
                                       cin_p, _st()))
    return gx32, gx16


def _im2col_s2(x: torch.Tensor, ks: int, reflect: int) -> torch.Tensor:
    """contiguous fp32 NCHW (n, c, h, w), k*k*c <= 32 -> bf16 columns [n][(h+1)/2][(w+1)/2][32] of its stride-2 windows (reflect
    1: the image under the reflect convolution; 0: an output gradient under the transposed one, zeros outside)"""
    n, c, h, w = x.shape
    assert ks * ks * c <= 32
    cols = _new(x, (n, (h + 1) // 2, (w + 1) // 2, 32), BF16)
    _lib.check(_L().cae_t_im2col_s2(x.data_ptr(), n, c, h, w, (h + 1) // 2, (w + 1) // 2, ks, reflect, cols.data_ptr(), _st()))
    return cols


def _col2im_s2(u32, bias_c, cout, ks):
    """fp32 columns [n][h][w][32] of the transposed stride-2 layer (+ bias, contiguous fp32 | None) -> NCHW (n, cout, 2h, 2w)"""
    n, h, w, cols = u32.shape
    assert cols == 32 and ks * ks * cout <= 32
    out = _new(u32, (n, cout, 2 * h, 2 * w), F32)
    _lib.check(_L().cae_t_col2im_s2(u32.data_ptr(), _ptr(bias_c), n, cout, h, w, ks, out.data_ptr(), _st()))
    return out


def _im2col_s1r(g: torch.Tensor, ks: int, kp: int) -> torch.Tensor:
    """contiguous fp32 NCHW output gradient of a colour layer -> its reflect-folded columns as a bf16 (hi, lo) pair,
    [n][h][w][2 kp]"""
    n, c, h, w = g.shape
    assert ks * ks * c <= kp
    gu16 = _new(g, (n, h, w, 2 * kp), BF16)
    _lib.check(_L().cae_t_im2col_s1r(g.data_ptr(), n, c, h, w, ks, kp, gu16.data_ptr(), _st()))
    return gu16


def _col2im_s1r(u32, bias_c, cout, ks):
    """fp32 columns [n][h][w][kp] of a colour layer (+ bias) -> NCHW (n, cout, h, w) under reflect padding"""
    n, h, w, kp = u32.shape
    assert ks * ks * cout <= kp
    out = _new(u32, (n, cout, h, w), F32)
    _lib.check(_L().cae_t_col2im_s1r(u32.data_ptr(), _ptr(bias_c), n, cout, h, w, ks, kp, out.data_ptr(), _st()))
    return out


def _gdn_fused(cp: int) -> bool:
    """one-kernel GDN forward (saving the factor f, y = z f) / backward (cae_t_gdn_*_save / _fused: up to 128 channels);
    CAE_GDN_FUSED=0 keeps the three-kernel backward, which the tests use as the comparison"""
    return cp <= 128 and os.environ.get('CAE_GDN_FUSED', '1') != '0'


def _gdn_forward(z32: torch.Tensor, beta_p: torch.Tensor, gamma_p: torch.Tensor, inverse: bool):
    """-> (y16, saved factor f | None)"""
    n, h, w, cp = z32.shape
    y16 = torch.empty_like(z32, dtype=BF16)
    beta, gamma = beta_p.detach().float().contiguous(), gamma_p.detach().float().contiguous()  # (alive across the call)
    if _gdn_fused(cp):
        f = _new(z32, _L().cae_t_gdn_saved_elems(n * h * w, cp), F32)
        _lib.check(_L().cae_t_gdn_forward_save(z32.data_ptr(), n * h * w, cp, beta.data_ptr(), gamma.data_ptr(),
                                               int(inverse), y16.data_ptr(), f.data_ptr(), _st()))
        return y16, f
    _lib.check(_L().cae_t_gdn_forward(z32.data_ptr(), n * h * w, cp, beta.data_ptr(), gamma.data_ptr(), int(inverse),
                                      None, y16.data_ptr(), _st()))
    return y16, None


def _gdn_backward(z32, gext32, pad, beta_p, gamma_p, inverse, f=None):
    """-> (gz16, g_beta_p, g_gamma_p)"""
    n, h, w, cp = z32.shape
    gz16 = torch.empty_like(z32, dtype=BF16)
    gg, gb = _new(z32, (cp, cp), F32), _new(z32, (cp,), F32)
    gamma = gamma_p.detach().float().contiguous()
    if f is not None:
        _lib.check(_L().cae_t_gdn_backward_fused(z32.data_ptr(), f.data_ptr(), gext32.data_ptr(), n, h, w, pad, cp,
                                                 gamma.data_ptr(), int(inverse), gz16.data_ptr(), gg.data_ptr(),
                                                 gb.data_ptr(), _st()))
        return gz16, gb, gg
    gn, gzd = torch.empty_like(z32), torch.empty_like(z32)
    gamma_t = gamma.t().contiguous()
    beta = beta_p.detach().float().contiguous()
    _lib.check(_L().cae_t_gdn_backward(z32.data_ptr(), gext32.data_ptr(), n, h, w, pad, cp,
                                       beta.data_ptr(), gamma.data_ptr(), gamma_t.data_ptr(),
                                       int(inverse), gn.data_ptr(), gzd.data_ptr(), None, gz16.data_ptr(), gg.data_ptr(),
                                       gb.data_ptr(), _st()))
    return gz16, gb, gg


def _bn_moments(a: torch.Tensor, b: torch.Tensor):
    """contiguous fp32 NCHW a, b -> per channel (sum a, sum a b) in float64"""
    n, c, h, w = a.shape
    assert b.shape == a.shape
    s1, s2 = _new(a, c, F64), _new(a, c, F64)
    _lib.check(_L().cae_t_bn_moments(a.data_ptr(), b.data_ptr(), n, c, h * w, s1.data_ptr(), s2.data_ptr(), _st()))
    return s1, s2


def _bn_affine(a: torch.Tensor, b: Optional[torch.Tensor], A: torch.Tensor, B: Optional[torch.Tensor], C: torch.Tensor):
    """-> a A + b B + C with per-channel fp32 coefficients (b, B: None without the second term)"""
    n, c, h, w = a.shape
    assert (b is None) == (B is None) and (b is None or b.shape == a.shape) and A.numel() == C.numel() == c
    out = torch.empty_like(a)
    _lib.check(_L().cae_t_bn_affine(a.data_ptr(), _ptr(b), n, c, h * w, A.data_ptr(), _ptr(B), C.data_ptr(), out.data_ptr(), _st()))
    return out


def _weight_grad(gw: torch.Tensor, spec_shape: Tuple[int, int], ks: int) -> torch.Tensor:
    """gw [k*k][ca][cb] -> gradient of a (d0 = b, d1 = a, k, k) weight"""
    d0, d1 = spec_shape
    return gw.permute(2, 1, 0)[:d0, :d1].reshape(d0, d1, ks, ks).contiguous()


# ---- steps shared by the fused tracks and the composed functions ------------------------------------------------------

def _conv_s1_forward(a16, w, b, ks, act, synthesis, want32, want16):
    """stride-1 convolution (+ bias) (+ activation): reflect Conv2d (analysis) or ConvTranspose2d(padding k//2)
    (synthesis) -> (fp32 output | None, bf16 output behind the activation | None)"""
    wp, bp = _pack_bias(w, b, 0 if synthesis else 1, ks)
    return _corr_s1(a16, wp, 2 if synthesis else 0, bp, act, want32, want16)


def _conv_s1_backward(gu16, a16, w, has_bias, synthesis, dgrad=True, want32=True):
    """backward of _conv_s1_forward from the bf16 gradient gu16 at its (pre-activation) output and its input a16
    -> (g_w, g_b | None, fp32 data gradient | None, bf16 data gradient | None); the analysis form's data gradient is fp32 on
    the extended domain (to be folded); dgrad False: the parameter gradients only"""
    ks = w.shape[2]
    gwp = _wgrad_s1(gu16, a16, ks, 0) if synthesis else _wgrad_s1(a16, gu16, ks, 1)
    g_w = _weight_grad(gwp, tuple(w.shape[:2]), ks)
    g_b = _colsum(gu16, w.shape[1 if synthesis else 0]) if has_bias else None
    if not dgrad:
        return g_w, g_b, None, None
    return (g_w, g_b) + _corr_s1(gu16, _pack(w, 1 if synthesis else 0, ks), 3 if synthesis else 1, want32=want32,
                                 want16=not want32)


def _conv_s2_backward(g16, x16, w, has_bias, dgrad=True):
    """backward of the strided reflect convolution (cout, cin, k, k) from the bf16 gradient at its output and its bf16 input
    -> (g_w, g_b | None, fp32 data gradient on the extended domain | None)"""
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    g_w = _weight_grad(_wgrad(x16, g16, ks, 1), (cout, cin), ks)
    g_b = _colsum(g16, cout) if has_bias else None
    return g_w, g_b, (_conv_dgrad_ext(g16, _pack(w, 0, ks), x16.shape[1:3]) if dgrad else None)


class _Saved(NamedTuple):
    """what one unit of a fused track keeps for its backward"""
    a_in: torch.Tensor            # bf16 input of the unit (edge first layer: the im2col columns of the image)
    p: Optional[torch.Tensor]     # bf16 output of the stride-1 pre-convolution (behind its activation)
    z: Optional[torch.Tensor]     # fp32 input of the GDN / IGDN
    f: Optional[torch.Tensor]     # the factor the fused GDN forward saved
    out: Optional[torch.Tensor]   # bf16 output behind the LeakyReLU / ReLU of a non-last unit
    edge: bool = False            # the 3-channel edge layer as a pointwise GEMM


def _layer_forward(conv, x16, wp, bias_p, s: LayerSpec, beta, gamma, last: bool, inverse: bool, a_in, p16, edge=False):
    """the strided layer `conv` (_conv_fwd / _deconv_fwd / _pointwise on x16) and what follows it: fp32 into a GDN / IGDN or
    out of the track, else bf16 behind the activation -> (bf16 input of the next unit, fp32 output | None, _Saved)"""
    need32 = s.has_gdn or last
    z32, z16 = conv(x16, wp, bias_p, 0 if need32 else s.act, need32)
    a16, f = _gdn_forward(z32, beta, gamma, inverse) if s.has_gdn else (z16, None)
    return a16, z32, _Saved(a_in, p16, z32 if s.has_gdn else None, f, z16 if s.act else None, edge)


def _hand_down(gx32, gx16, pad, prev: LayerSpec, sv: _Saved, beta_p, gamma_p, inverse: bool, colour=None):
    """a level's data gradient -> the bf16 gradient at the previous unit's strided layer.  gx32: fp32, extended by `pad`
    (analysis: the reflect border is folded by whichever kernel reads it; synthesis: 0), or None with gx16 already rounded
    (nothing between the two layers).  colour = (g, a16, cs, w, has_bias) of the level's colour layer: its data gradient is
    added to gx32 first, so the level's gradient is rounded once.  Through the previous unit's GDN / IGDN, or its
    LeakyReLU / ReLU mask, or the plain fold / rounding -> (g16, g_beta | None, g_gamma | None, colour (g_w, g_b) | None)"""
    col = _colour_backward(*colour, gx32) if colour is not None else None
    if prev.has_gdn:
        return _gdn_backward(sv.z, gx32, pad, beta_p, gamma_p, inverse, sv.f) + (col,)
    if sv.out is not None:
        return _act_backward(None, gx32, pad, sv.out, prev.act), None, None, col
    return (gx16 if gx32 is None else _fold_to_bf16(gx32, pad)), None, None, col


def _colour_forward(a16: torch.Tensor, cs: ColourSpec, wt: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """colour layer on a level's bf16 activation [n][h][w][cin_p] -> NCHW fp32 (n, cout, h, w)"""
    n, h, w, cp = a16.shape
    P = cs.ks // 2
    if h <= P or w <= P:
        raise ValueError(f'colour layer: a {h} x {w} level is too small for reflect padding {P}')
    if _colour_edge(cs):
        # u[q][(tap, co)] = sum_ci a[q][ci] W[co][ci][tap] (1 x 1 GEMM, N = kp), then the reflect col2im + bias
        u32, _ = _pointwise(a16, _colour_1x1(wt, cs, False), None, 0, True)
        return _col2im_s1r(u32, None if b is None else b.detach().float().contiguous(), cs.cout, cs.ks)
    return _to_nchw(_conv_s1_forward(a16, wt, b, cs.ks, 0, False, True, False)[0], cs.cout)


def _colour_backward(g: torch.Tensor, a16: torch.Tensor, cs: ColourSpec, wt: torch.Tensor, has_bias: bool,
                     acc32: torch.Tensor):
    """gradient of a colour layer's NCHW output g: its data gradient is ADDED to acc32 (fp32 [n][h][w][cin_p], the level's
    gradient); -> (g_w, g_b | None)"""
    gc = g.detach().float().contiguous()
    g_b = gc.bfloat16().float().sum(dim=(0, 2, 3)) if has_bias else None
    if _colour_edge(cs):
        # gu = the folded output gradient as a bf16 (hi, lo) pair: 2 kp GEMM columns, the weights repeated over both halves
        gu16 = _im2col_s1r(gc, cs.ks, cs.kp)
        gw1 = _wgrad_pointwise(a16, gu16)
        gw = gw1[0, :cs.cin, :cs.K] + gw1[0, :cs.cin, cs.kp:cs.kp + cs.K]
        g_w = gw.reshape(cs.cin, cs.ks, cs.ks, cs.cout).permute(3, 0, 1, 2).contiguous()
        _pointwise_acc(gu16, _colour_1x1(wt, cs, True), acc32)
        return g_w, g_b
    gu16, _ = _from_nchw(gc, _pad32(cs.cout))
    g_w, _, gext, _ = _conv_s1_backward(gu16, a16, wt, False, False)
    _fold_acc(gext, cs.ks // 2, acc32)
    return g_w, g_b


class AnalysisFn(torch.autograd.Function):
    """Analyzer.forward under autograd: L x [(conv s1 + act)? reflect conv s2 (+bias) (+GDN | act)]
    (_autoencoders.py:62-85, :29-30)."""

    @staticmethod
    def forward(ctx, x, specs, *tensors):
        layers = _split_params(specs, tensors)
        edge = _edge_ok(specs[0], specs[0].cin)
        a16 = None if edge else _from_nchw(x, specs[0].cin_p)[0]
        saved = []
        for i, (s, (wt, b, beta, gamma, pw, pb)) in enumerate(zip(specs, layers)):
            last = i == len(specs) - 1
            if i == 0 and edge:
                # first layer: K = (tap, channel) = 27 of 32 as ONE contraction chunk of a 1 x 1 GEMM on the im2col of the image
                cols = _im2col_s2(x.detach().float().contiguous(), s.ks, 1)
                a16, z32, sv = _layer_forward(_pointwise, cols, _first_layer_1x1(wt, s), _bias_p(b, s.cout_p, x.device), s,
                                              beta, gamma, last, False, cols, None, edge=True)
            else:
                p16 = _conv_s1_forward(a16, pw, pb, s.ks, s.act, False, False, True)[1] if s.has_pre else None
                a16, z32, sv = _layer_forward(_conv_fwd, a16 if p16 is None else p16, *_pack_bias(wt, b, 1, s.ks), s,
                                              beta, gamma, last, False, a16, p16)
            saved.append(sv)
        ctx.specs, ctx.saved, ctx.layers = specs, saved, _detached(layers)
        return _to_nchw(z32, specs[-1].cout)

    @staticmethod
    def backward(ctx, gy):
        specs, saved, layers = ctx.specs, ctx.saved, ctx.layers
        g16, _ = _from_nchw(gy, specs[-1].cout_p)  # gradient with respect to the last convolution's output
        per_layer = [[None] * 6 for _ in specs]
        for i in reversed(range(len(specs))):
            s, sv = specs[i], saved[i]
            wt, b, _, _, pw, pb = layers[i]
            P = s.ks // 2
            if sv.edge:  # first layer as a pointwise GEMM: its weight gradient over the im2col, back in (cout, cin, k, k)
                gw1 = _wgrad_pointwise(sv.a_in, g16)
                per_layer[i][0] = (gw1[0, :s.ks * s.ks * s.cin, :s.cout].t().reshape(s.cout, s.ks, s.ks, s.cin)
                                   .permute(0, 3, 1, 2).contiguous())
                if b is not None:
                    per_layer[i][1] = _colsum(g16, s.cout)
                break  # (the image itself needs no gradient)
            per_layer[i][0], per_layer[i][1], gext = _conv_s2_backward(g16, sv.a_in if sv.p is None else sv.p, wt,
                                                                        b is not None, dgrad=i > 0 or s.has_pre)
            if s.has_pre:
                gu16 = _act_backward(None, gext, P, sv.p, s.act)  # fold + activation mask: gradient at the pre-convolution's output
                per_layer[i][4], per_layer[i][5], gext, _ = _conv_s1_backward(gu16, sv.a_in, pw, pb is not None, False,
                                                                               dgrad=i > 0)
            if i == 0:
                break  # (the image itself needs no gradient)
            _, _, beta_p, gamma_p, _, _ = layers[i - 1]
            g16, per_layer[i - 1][2], per_layer[i - 1][3], _ = _hand_down(gext, None, P, specs[i - 1], saved[i - 1],
                                                                          beta_p, gamma_p, False)
        return (None, None, *_flat_grads(specs, per_layer))


class SynthesisFn(torch.autograd.Function):
    """Synthesizer.forward under autograd: L x [(conv-transpose s1 + act)? conv-transpose s2 (+bias) (+IGDN | act)]
    (_autoencoders.py:187-211).  `colour` (multiscale_analysis, :417-452): one ColourSpec per non-last level, their weights
    (and biases) after the track's tensors; each reads the level's bf16 activation (what the next unit reads) and the
    function returns (x_r, colour_0 .. colour_{L-2}).  In the backward a colour layer's data gradient is added to the
    next unit's fp32 data gradient before the level's IGDN / activation backward (one rounding)."""

    @staticmethod
    def forward(ctx, yq, specs, colour, *tensors):
        nt = sum(s.n_tensors for s in specs)
        layers = _split_params(specs, tensors[:nt])
        col_layers = _split_colour(colour, tensors[nt:]) if colour else []
        colours, saved = [], []
        a16, _ = _from_nchw(yq, specs[0].cin_p)
        if colour:
            ctx.set_materialize_grads(False)  # (colour outputs the loss does not read hand back None)
        for i, (s, (wt, b, beta, gamma, pw, pb)) in enumerate(zip(specs, layers)):
            last = i == len(specs) - 1
            if colour and i > 0:  # colour layer of the previous level, on the activation this unit reads
                colours.append(_colour_forward(a16, colour[i - 1], *col_layers[i - 1]))
            # ConvTranspose2d(cin, cin, k, stride 1, padding k//2) + activation in front of LeakyReLU / ReLU units
            p16 = _conv_s1_forward(a16, pw, pb, s.ks, s.act, True, False, True)[1] if s.has_pre else None
            main_in = a16 if p16 is None else p16
            if last and _edge_ok(s, s.cout):
                # last layer: per INPUT position the k*k*cout <= 32 products with the weights (a 1 x 1 GEMM), then col2im
                u32, _ = _pointwise(main_in, _last_layer_1x1(wt, s, False), None, 0, True)
                x_r = _col2im_s2(u32, None if b is None else b.detach().float().contiguous(), s.cout, s.ks)
                saved.append(_Saved(a16, p16, None, None, None, edge=True))
            else:
                a16, z32, sv = _layer_forward(_deconv_fwd, main_in, *_pack_bias(wt, b, 0, s.ks), s, beta, gamma, last, True,
                                              a16, p16)
                saved.append(sv)
                if last:
                    x_r = _to_nchw(z32, s.cout)
        ctx.specs, ctx.saved, ctx.layers = specs, saved, _detached(layers)
        ctx.colour, ctx.col_layers = colour or None, [(cw.detach(), cb) for cw, cb in col_layers]
        ctx.need_input_grad, ctx.out_shape, ctx.dev = yq.requires_grad, tuple(x_r.shape), yq.device
        return (x_r, *colours) if colour else x_r

    @staticmethod
    def backward(ctx, gx, *gcols):
        specs, saved, layers = ctx.specs, ctx.saved, ctx.layers
        colour, col_layers = ctx.colour, ctx.col_layers
        if gx is None:
            gx = torch.zeros(ctx.out_shape, dtype=F32, device=ctx.dev)
        col_grads = [(None, None)] * (len(colour) if colour else 0)
        g16 = None if saved[-1].edge else _from_nchw(gx, specs[-1].cout_p)[0]  # gradient with respect to the last layer's output
        per_layer = [[None] * 6 for _ in specs]
        g_in = None
        for i in reversed(range(len(specs))):
            s, sv = specs[i], saved[i]
            wt, b, _, _, pw, pb = layers[i]
            main_in = sv.a_in if sv.p is None else sv.p
            stop = i == 0 and not ctx.need_input_grad
            has_col = i > 0 and colour is not None and gcols[i - 1] is not None
            # fp32 wherever something still reads the level's gradient before it is rounded (one rounding)
            want32 = i == 0 or has_col or specs[i - 1].has_gdn or saved[i - 1].out is not None
            if sv.edge:
                # last layer as a pointwise GEMM: gu[pos][(tap, co)] = g_x[2 pos - P + tap][co] (im2col of the output
                # gradient, zeros outside); weight gradient and data gradient are 1 x 1 contractions with it
                gxc = gx.detach().float().contiguous()
                gu16 = _im2col_s2(gxc, s.ks, 0)
                gw1 = _wgrad_pointwise(main_in, gu16)
                per_layer[i][0] = (gw1[0, :s.cin, :s.ks * s.ks * s.cout].reshape(s.cin, s.ks, s.ks, s.cout)
                                   .permute(0, 3, 1, 2).contiguous())
                if b is not None:
                    per_layer[i][1] = gxc.bfloat16().float().sum(dim=(0, 2, 3))
                if stop:
                    break
                gx32, gx16 = _pointwise(gu16, _last_layer_1x1(wt, s, True), None, 0, want32)
            else:
                per_layer[i][0] = _weight_grad(_wgrad(g16, main_in, s.ks, 0), (s.cin, s.cout), s.ks)
                if b is not None:
                    per_layer[i][1] = _colsum(g16, s.cout)
                if stop and not s.has_pre:
                    break
                gx32, gx16 = _deconv_dgrad(g16, _pack(wt, 1, s.ks), want32 or s.has_pre)
                if s.has_pre:
                    gu16 = _act_backward(None, gx32, 0, sv.p, s.act)  # gradient at the pre-convolution's output
                    per_layer[i][4], per_layer[i][5], gx32, gx16 = _conv_s1_backward(gu16, sv.a_in, pw, pb is not None, True,
                                                                                     dgrad=not stop, want32=want32)
                    if stop:
                        break
            if i == 0:
                g_in = _to_nchw(gx32, s.cin)
                break
            _, _, beta_p, gamma_p, _, _ = layers[i - 1]
            cw, cb = col_layers[i - 1] if has_col else (None, None)
            g16, per_layer[i - 1][2], per_layer[i - 1][3], col = _hand_down(
                gx32, gx16, 0, specs[i - 1], saved[i - 1], beta_p, gamma_p, True,
                (gcols[i - 1], sv.a_in, colour[i - 1], cw, cb is not None) if has_col else None)
            if has_col:
                col_grads[i - 1] = col
        flat_col = [g for cs, (g_w, g_b) in zip(colour or (), col_grads) for g in ((g_w, g_b) if cs.has_bias else (g_w,))]
        return (g_in, None, None, *_flat_grads(specs, per_layer), *flat_col)


# ---- residual units (ResidualDownsamplingUnit / ResidualUpsamplingUnit, _autoencoders.py:104-174, :230-304) ----------
# and units with batch norm: their tracks are composed per operation, on NCHW fp32 tensors between operations: every
# convolution, GDN and batch norm is one of the kernels behind a small autograd function of its own, the residual sum and
# stand-alone LeakyReLU / ReLU modules are element-wise torch operations on the unit's tensors.  (The canonical tracks keep their
# fused functions above; this form pays two layout conversions per operation.)

class _ConvS1Fn(torch.autograd.Function):
    """Stride-1 convolution cin -> cin of a residual unit's res_model, (+ bias) (+ LeakyReLU / ReLU): analysis = Conv2d with
    reflect padding, synthesis = ConvTranspose2d(stride 1, padding k//2) (_conv_s1_forward / _conv_s1_backward)."""

    @staticmethod
    def forward(ctx, x, synthesis, ks, act, w, b):
        c = x.shape[1]
        a16, _ = _from_nchw(x, _pad32(c))
        out32, out16 = _conv_s1_forward(a16, w, b, ks, act, synthesis, True, bool(act))
        ctx.a16, ctx.out16, ctx.w = a16, out16, w.detach()
        ctx.cfg = (bool(synthesis), int(ks), int(act), b is not None, c)
        return _to_nchw(out32, c)

    @staticmethod
    def backward(ctx, g):
        synthesis, ks, act, has_bias, c = ctx.cfg
        cp = ctx.a16.shape[3]
        if act:  # through the activation on the fp32 gradient (one rounding)
            gu16 = _act_backward(None, _from_nchw(g, cp, want16=False, want32=True)[1], 0, ctx.out16, act)
        else:
            gu16 = _from_nchw(g, cp)[0]
        g_w, g_b, gx32, _ = _conv_s1_backward(gu16, ctx.a16, ctx.w, has_bias, synthesis)
        if not synthesis:  # extended domain: the reflect fold
            gx32 = _fold_to_bf16(gx32, ks // 2).float()
        return _to_nchw(gx32, c), None, None, None, g_w, g_b


class _ConvS2Fn(torch.autograd.Function):
    """The strided reflect convolution of an analysis unit alone, with its input gradient (AnalysisFn's first layer reads the
    image and returns none)."""

    @staticmethod
    def forward(ctx, x, ks, w, b):
        a16, _ = _from_nchw(x, _pad32(x.shape[1]))
        z32, _ = _conv_fwd(a16, *_pack_bias(w, b, 1, ks), 0, True)
        ctx.a16, ctx.w, ctx.cfg = a16, w.detach(), (int(ks), b is not None)
        return _to_nchw(z32, w.shape[0])

    @staticmethod
    def backward(ctx, g):
        ks, has_bias = ctx.cfg
        cout, c = ctx.w.shape[0], ctx.w.shape[1]
        g_w, g_b, gext = _conv_s2_backward(_from_nchw(g, _pad32(cout))[0], ctx.a16, ctx.w, has_bias)
        return _to_nchw(_fold_to_bf16(gext, ks // 2).float(), c), None, g_w, g_b


class _GdnFn(torch.autograd.Function):
    """GDN / IGDN alone on an NCHW fp32 tensor (effective, padded beta / gamma): the fused forward / backward kernels."""

    @staticmethod
    def forward(ctx, x, inverse, beta_p, gamma_p):
        c, cp = x.shape[1], beta_p.numel()
        z32 = _from_nchw(x, cp, want16=False, want32=True)[1]
        y16, f = _gdn_forward(z32, beta_p, gamma_p, bool(inverse))
        ctx.z32, ctx.f, ctx.beta_p, ctx.gamma_p, ctx.cfg = z32, f, beta_p.detach(), gamma_p.detach(), (bool(inverse), c)
        return _to_nchw(y16.float(), c)

    @staticmethod
    def backward(ctx, g):
        inverse, c = ctx.cfg
        cp = ctx.beta_p.numel()
        g32 = _from_nchw(g, cp, want16=False, want32=True)[1]  # (the backward kernel works in this buffer)
        gz16, g_beta, g_gamma = _gdn_backward(ctx.z32, g32, 0, ctx.beta_p, ctx.gamma_p, inverse, ctx.f)
        return _to_nchw(gz16.float(), c), None, g_beta, g_gamma


def _gdn_params(g, c: int):
    """effective, padded (beta, gamma) of a GDN module, in the autograd graph (LowerBound gradient rule inside)"""
    cp = _pad32(c)
    beta, gamma = g.beta_reparam(g.beta), g.gamma_reparam(g.gamma)
    beta_p = torch.cat([beta, beta.new_ones(cp - c)]) if cp > c else beta
    gamma_p = torch.nn.functional.pad(gamma, (0, cp - c, 0, cp - c)) if cp > c else gamma
    return beta_p, gamma_p


class _BatchNormFn(torch.autograd.Function):
    """nn.BatchNorm2d in training mode on an NCHW fp32 tensor: batch statistics (biased variance for the normalisation, as
    torch) by cae_t_bn_moments, y = x w rstd + (b - mean w rstd) by cae_t_bn_affine; the backward is the same pair of kernels
    with dy (the per-channel coefficients are C-element float64 arithmetic).  -> (y, batch mean, biased batch variance)"""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.detach().float().contiguous()
        n, c, h, w = x.shape
        s1, s2 = _bn_moments(x, x)
        m = float(n * h * w)
        mean = s1 / m
        var = (s2 / m - mean * mean).clamp_min(0.0)
        rstd = torch.rsqrt(var + eps)
        wt = weight.detach().double() if weight is not None else torch.ones(c, dtype=F64, device=x.device)
        bs = bias.detach().double() if bias is not None else torch.zeros(c, dtype=F64, device=x.device)
        y = _bn_affine(x, None, (wt * rstd).float().contiguous(), None, (bs - mean * wt * rstd).float().contiguous())
        ctx.x, ctx.stats, ctx.has = x, (mean, rstd, wt, m), (weight is not None, bias is not None)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _gm, _gv):
        x = ctx.x
        mean, rstd, wt, m = ctx.stats
        dy = dy.detach().float().contiguous()
        s1, s2 = _bn_moments(dy, x)
        sdyx = (s2 - mean * s1) * rstd  # sum dy xhat
        # dx = w rstd (dy - sum(dy) / m - xhat sum(dy xhat) / m),  xhat = (x - mean) rstd
        A = (wt * rstd).float().contiguous()
        B = (-wt * rstd * rstd * sdyx / m).float().contiguous()
        C = (wt * rstd * (-s1 / m + mean * rstd * sdyx / m)).float().contiguous()
        dx = _bn_affine(dy, x, A, B, C)
        has_w, has_b = ctx.has
        return dx, (sdyx.float() if has_w else None), (s1.float() if has_b else None), None


def _batch_norm(bn: nn.BatchNorm2d, x: torch.Tensor) -> torch.Tensor:
    """bn(x) in training mode, with the running statistics updated as nn.BatchNorm2d does (unbiased variance, momentum or
    the cumulative average when momentum is None)."""
    y, mean, var = _BatchNormFn.apply(x, bn.weight, bn.bias, bn.eps)
    if bn.track_running_stats and bn.running_mean is not None:
        with torch.no_grad():
            bn.num_batches_tracked += 1
            mom = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            cnt = x.numel() / x.shape[1]
            bn.running_mean.mul_(1.0 - mom).add_(mean.to(bn.running_mean.dtype), alpha=mom)
            bn.running_var.mul_(1.0 - mom).add_((var * (cnt / max(cnt - 1.0, 1.0))).to(bn.running_var.dtype), alpha=mom)
    return y


def _dense_weight(m) -> torch.Tensor:
    """The dense (groups = 1) weight of a grouped layer as a differentiable function of its parameter: block-diagonal
    embedding by one index_put (modules._ConvParams.dense_weight is its no-grad twin for the inference upload); the
    gradient of the grouped weight is the block diagonal of the dense kernels' weight gradient."""
    w = m.weight
    if m.groups == 1:
        return w
    g, k = m.groups, m.kernel_size
    cin_g, cout_g = m.in_channels // g, m.out_channels // g
    dev = w.device
    if m.transposed:  # (cin, cout_g, k, k) -> (cin, cout, k, k)
        rows = torch.arange(m.in_channels, device=dev)
        cols = (rows // cin_g)[:, None] * cout_g + torch.arange(cout_g, device=dev)[None, :]
        dense = w.new_zeros(m.in_channels, m.out_channels, k, k)
    else:             # (cout, cin_g, k, k) -> (cout, cin, k, k)
        rows = torch.arange(m.out_channels, device=dev)
        cols = (rows // cout_g)[:, None] * cin_g + torch.arange(cin_g, device=dev)[None, :]
        dense = w.new_zeros(m.out_channels, m.in_channels, k, k)
    return dense.index_put((rows[:, None].expand_as(cols), cols), w)


class _ColourFn(torch.autograd.Function):
    """A multiscale colour layer alone on an NCHW fp32 level (composed tracks): the forms of _colour_forward /
    _colour_backward."""

    @staticmethod
    def forward(ctx, x, cs, w, b):
        a16, _ = _from_nchw(x, cs.cin_p)
        ctx.a16, ctx.cs, ctx.w = a16, cs, w.detach()
        return _colour_forward(a16, cs, w, b)

    @staticmethod
    def backward(ctx, g):
        cs = ctx.cs
        gx32 = torch.zeros(ctx.a16.shape, dtype=torch.float32, device=ctx.a16.device)
        g_w, g_b = _colour_backward(g, ctx.a16, cs, ctx.w, cs.has_bias, gx32)
        return _to_nchw(gx32, cs.cin), None, g_w, g_b


def _run_sequence(u, seq, x: torch.Tensor, synthesis: bool) -> torch.Tensor:
    """The modules of a unit's nn.Sequential, one operation each (the module order IS the reference's forward)."""
    from .modules import GDN, _ConvParams
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, _ConvParams):
            wd = _dense_weight(m)  # (grouped layers: the dense kernels on the block-diagonal embedding)
            if m is u.main:  # the strided layer
                if synthesis:
                    spec = LayerSpec(m.in_channels, m.out_channels, m.kernel_size, m.bias is not None, False)
                    x = SynthesisFn.apply(x, (spec,), None, *([wd] + ([m.bias] if m.bias is not None else [])))
                else:
                    x = _ConvS2Fn.apply(x, m.kernel_size, wd, m.bias)
            else:  # stride 1; a LeakyReLU / ReLU right behind it rides in the kernel's epilogue
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                act = 1 if isinstance(nxt, nn.LeakyReLU) else (2 if isinstance(nxt, nn.ReLU) else 0)
                x = _ConvS1Fn.apply(x, synthesis, m.kernel_size, act, wd, m.bias)
                i += 1 if act else 0
        elif isinstance(m, nn.BatchNorm2d):
            x = _batch_norm(m, x) if m.training else m(x)
        elif isinstance(m, GDN):
            x = _GdnFn.apply(x, m.inverse, *_gdn_params(m, m.in_channels))
        elif isinstance(m, nn.LeakyReLU):
            x = torch.nn.functional.leaky_relu(x, m.negative_slope)
        elif isinstance(m, nn.ReLU):
            x = torch.relu(x)
        elif isinstance(m, nn.Dropout2d):
            x = m(x)  # (channel mask from torch's generator, as in the reference; the identity in eval mode)
        elif not isinstance(m, nn.Identity):
            raise NotImplementedError(f'{type(m).__name__} is not part of the compression path')
        i += 1
    return x


def _composed_track(units, x: torch.Tensor, synthesis: bool, colour=None, ctensors=()):
    """Tracks with residual units (y = model(res_model(x) + x), _autoencoders.py:168-174, :298-304) or batch norm:
    composed per operation.  With `colour` (synthesis, multiscale): -> (x, [colour_0 .. colour_{L-2}])."""
    from .modules import _ResidualUnit
    col_layers = _split_colour(colour, ctensors) if colour else []
    cols = []
    for i, u in enumerate(units):
        if isinstance(u, _ResidualUnit):
            x = _run_sequence(u, u.model, _run_sequence(u, u.res_model, x, synthesis) + x, synthesis)
        else:
            x = _run_sequence(u, u.model, x, synthesis)
        if colour and i < len(units) - 1:
            cols.append(_ColourFn.apply(x, colour[i], *col_layers[i]))
    return (x, cols) if colour is not None else x


def _track_inputs(track, units, synthesis: bool):
    """-> (specs, flat tensor list) of a track; effective, padded GDN parameters stay in the autograd graph."""
    from .modules import _ResidualUnit
    specs, tensors = [], []
    for u in units:
        if (isinstance(u, _ResidualUnit) or u.main_bn_index is not None or u.pre_bn_index is not None or u.main.groups != 1
                or any(isinstance(m, nn.Dropout2d) and m.p > 0 for m in u.model)):
            return None, None  # composed per operation: _composed_track
        conv = u.main
        specs.append(LayerSpec(conv.in_channels, conv.out_channels, conv.kernel_size, conv.bias is not None, u.gdn is not None,
                               act=u.act_code, has_pre=u.pre is not None))
        if u.pre is not None:  # LeakyReLU / ReLU units: the stride-1 convolution in front (same bias setting as the layer)
            tensors.append(u.pre.weight)
            if conv.bias is not None:
                tensors.append(u.pre.bias)
        tensors.append(conv.weight)
        if conv.bias is not None:
            tensors.append(conv.bias)
        if u.gdn is not None:
            tensors.extend(_gdn_params(u.gdn, conv.out_channels))
    return tuple(specs), tensors


def _colour_inputs(track, units):
    """-> (ColourSpec per non-last level, flat weight / bias list) of a multiscale synthesis track, (None, []) without
    multiscale_analysis.  Grouped colour layers (groups = channels_org) as the dense weight (_dense_weight)."""
    if not getattr(track, 'multiscale_analysis', False):
        return None, []
    specs, tensors = [], []
    for i, layer in enumerate(list(track.color_layers)[:len(units) - 1]):
        conv = layer[0]
        if conv.in_channels != units[i].main.out_channels:  # (the reference's own channel plan, channels_expansion != 1)
            raise NotImplementedError(f'colour layer {i} expects {conv.in_channels} input channels, the level produces '
                                      f'{units[i].main.out_channels}')
        specs.append(ColourSpec(conv.in_channels, conv.out_channels, conv.kernel_size, conv.bias is not None))
        tensors.append(_dense_weight(conv))
        if conv.bias is not None:
            tensors.append(conv.bias)
    return tuple(specs), tensors


def needs_grad(module: nn.Module, x: torch.Tensor) -> bool:
    """The differentiable track functions run when the module is in TRAINING mode and autograd is recording
    (train_cae_ms.py:183-187 puts the trainable modules in train(), the others in eval() under fixed_module's no_grad).
    In eval mode the inference kernels run whether or not autograd is enabled: the reference's codec.encode forgets
    torch.no_grad() (_autoencoders.py:539-555) and must keep its inference numerics."""
    if not (module.training and torch.is_grad_enabled()):
        return False
    return x.requires_grad or any(p.requires_grad for p in module.parameters())


def analysis_forward(track, x: torch.Tensor) -> torch.Tensor:
    dev = _lib.require_gpu()
    specs, tensors = _track_inputs(track, track._units(), False)
    x = x.to(device=dev, dtype=torch.float32)
    if specs is None:
        return _composed_track(track._units(), x, False)
    return AnalysisFn.apply(x, specs, *tensors)


def synthesis_forward(track, yq: torch.Tensor):
    dev = _lib.require_gpu()
    units = track._units()
    specs, tensors = _track_inputs(track, units, True)
    colour, ctensors = _colour_inputs(track, units)
    yq = yq.to(device=dev, dtype=torch.float32)
    cols: List[torch.Tensor] = []
    if specs is None:
        out = _composed_track(units, yq, True, colour, ctensors)
        if colour is not None:
            out, cols = out
    elif colour:
        out, *cols = SynthesisFn.apply(yq, specs, colour, *tensors, *ctensors)
    else:
        out = SynthesisFn.apply(yq, specs, None, *tensors)
    L = len(units)
    # (x_r list, fx_brg) as the reference's Synthesizer: x_r = [out, colour_{L-2}, ..., colour_0] (None without
    # multiscale_analysis); intermediate features are not materialised while training
    return [out] + (cols[::-1] if cols else [None] * (L - 1)), [None] * (L - 1) + [out]


# ---- optimisers and the training step (train_cae_ms.py) -----------------------------------------------------------

def setup_optim(model: Dict[str, nn.Module], trainable_modules: Sequence[str] = ('encoder', 'decoder', 'fact_ent'),
                learning_rate: float = 1e-4, aux_learning_rate: float = 1e-3, weight_decay: float = 0.0,
                algo=torch.optim.Adam, capturable: bool = False) -> Dict[str, torch.optim.Optimizer]:
    """One optimiser per trainable module; parameters whose name contains 'quantiles' or 'aux' go to a separate
    ``<module>_aux`` optimiser (train_cae_ms.py:584-641).  capturable: step counters on the device (no host read per
    step)."""
    opts: Dict[str, torch.optim.Optimizer] = {}
    extra = dict(capturable=True) if capturable else {}
    for k in trainable_modules:
        pars, aux = [], []
        for name, par in model[k].named_parameters():
            (aux if ('quantiles' in name.lower() or 'aux' in name.lower()) else pars).append(par)
        opts[k] = algo([dict(params=pars, lr=learning_rate, weight_decay=weight_decay)], **extra)
        if aux:
            opts[k + '_aux'] = algo([dict(params=aux, lr=aux_learning_rate, weight_decay=weight_decay)], **extra)
    return opts


_OPTIM_WS: Dict[torch.device, torch.Tensor] = {}


def fused_clip_adam(optimizers: Dict[str, torch.optim.Optimizer], max_norm: float = 1.0) -> bool:
    """`for opt: clip_grad_norm_(params, max_norm); opt.step(); opt.zero_grad()` (train_cae_ms.py:221-230) for ALL
    optimisers in two launches (cae_t_clip_adam), on the optimisers' own state tensors (exp_avg, exp_avg_sq, step), so
    `state_dict()` / checkpoints stay torch.optim.Adam's.  -> False (nothing done) unless every optimiser is a plain
    torch.optim.Adam (one parameter group, no amsgrad / maximize / capturable) over contiguous fp32 CUDA parameters;
    CAE_FUSED_OPTIM=0 disables it."""
    if os.environ.get('CAE_FUSED_OPTIM', '1') == '0' or len(optimizers) > 8:
        return False
    items = []  # (p, grad, exp_avg, exp_avg_sq, group index)
    groups = []
    for gi, opt in enumerate(optimizers.values()):
        if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
            return False
        g = opt.param_groups[0]
        if g.get('amsgrad') or g.get('maximize') or g.get('capturable') or g.get('differentiable') or \
                not isinstance(g['lr'], (int, float)):
            return False
        live = [p for p in g['params'] if p.grad is not None]
        for p in live:
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.grad.dtype != torch.float32:
                return False
        groups.append((opt, g, live))
    for gi, (opt, g, live) in enumerate(groups):
        for p in live:
            st = opt.state[p]
            if len(st) == 0:  # as torch.optim.Adam initialises it lazily
                st['step'] = torch.tensor(0.0)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not (st['exp_avg'].is_contiguous() and st['exp_avg_sq'].is_contiguous()) or st['step'].is_cuda:
                return False
            items.append((p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), st['exp_avg'], st['exp_avg_sq'], gi))
    if not items or len(items) > 64:
        return False
    n, G = len(items), len(groups)
    steps = []
    for opt, g, live in groups:
        steps.append(int(opt.state[live[0]]['step'].item()) + 1 if live else 1)
        for p in live:
            opt.state[p]['step'] += 1
    vp = lambda k: (ctypes.c_void_p * n)(*[it[k].data_ptr() for it in items])  # noqa: E731
    numel = (ctypes.c_int * n)(*[it[0].numel() for it in items])
    grp = (ctypes.c_int * n)(*[it[4] for it in items])
    fl = lambda vals: (ctypes.c_float * G)(*vals)  # noqa: E731
    chunks = sum((it[0].numel() + 2047) // 2048 for it in items)
    dev = items[0][0].device
    ws = _OPTIM_WS.get(dev)
    if ws is None or ws.numel() < chunks:
        ws = _OPTIM_WS[dev] = torch.empty(max(chunks, 1024), dtype=torch.float32, device=dev)
    _lib.check(_L().cae_t_clip_adam(
        n, vp(0), vp(1), vp(2), vp(3), numel, grp, G, fl([g['lr'] for _, g, _ in groups]),
        fl([g['betas'][0] for _, g, _ in groups]), fl([g['betas'][1] for _, g, _ in groups]), fl([g['eps'] for _, g, _ in groups]),
        fl([g['weight_decay'] for _, g, _ in groups]), fl([max_norm] * G), (ctypes.c_int * G)(*steps), ws.data_ptr(), ws.numel(),
        _st()))
    for opt, g, _ in groups:  # zero_grad(set_to_none=True)
        for p in g['params']:
            p.grad = None
    return True


def train_step(x: torch.Tensor, model, criterion, optimizers, forward_func=None, reducer: 'GradReducer' = None):
    """One iteration of the reference's hot loop (train_cae_ms.py:209-230).  -> loss_dict (detached scalars)"""
    from .criteria import setup_forward_func
    forward_func = forward_func or setup_forward_func()
    output = forward_func(x, model)
    loss_dict = criterion(inputs=x, outputs=output, net=model)
    loss = torch.mean(loss_dict['loss'])
    loss.backward()
    if 'entropy_loss' in loss_dict:
        torch.mean(loss_dict['entropy_loss']).backward()
    if reducer is not None:
        reducer.reduce()
    if not fused_clip_adam(optimizers, max_norm=1.0):
        for opt in optimizers.values():
            nn.utils.clip_grad_norm_(opt.param_groups[0]['params'], max_norm=1.0)
            opt.step()
            opt.zero_grad()
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in loss_dict.items()}


class GradReducer:
    """Data-parallel gradient averaging, one process per GPU (replaces nn.DataParallel's reduce-add to device 0,
    _autoencoders.py:517): the gradients are packed into a few flat fp32 buckets and all-reduced (RCCL over xGMI on GPUs,
    gloo in the CPU tests), averaged, and handed back as views of the bucket.  OVERLAPPED with the backward pass: a
    post-accumulate hook per parameter counts a bucket down and launches its all-reduce (async) the moment its last
    gradient exists -- the backward runs decoder, entropy model, encoder, so the decoder's bucket is on the wire while the
    encoder's gradients are still being computed; ``reduce()`` (between ``backward()`` and the optimiser step) launches
    what is left (parameters without a gradient count as zero), waits and averages.  The buckets are persistent: no
    per-step concatenation.  The model holds about 2 M parameters (8 MB): latency-bound, a single ring."""

    def __init__(self, params: Sequence[torch.Tensor], bucket_bytes: int = 2 << 20, overlap: bool = True):
        self.params = [p for p in params if p.requires_grad]
        self.buckets: List[List[torch.Tensor]] = [[]]
        size = 0
        for p in self.params:
            nbytes = p.numel() * 4
            if size + nbytes > bucket_bytes and self.buckets[-1]:
                self.buckets.append([])
                size = 0
            self.buckets[-1].append(p)
            size += nbytes
        self._flat: List[Optional[torch.Tensor]] = [None] * len(self.buckets)
        self._views: List[Optional[List[torch.Tensor]]] = [None] * len(self.buckets)
        self._works: List = [None] * len(self.buckets)
        self._pending = [len(b) for b in self.buckets]
        self._bucket_of = {id(p): i for i, b in enumerate(self.buckets) for p in b}
        self.launched_in_backward = 0  # (statistics: buckets whose all-reduce started from a hook)
        self._hooks = []
        if overlap and hasattr(torch.Tensor, 'register_post_accumulate_grad_hook'):
            for p in self.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))

    @staticmethod
    def _active() -> bool:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def _on_grad(self, p):
        if not self._active():
            return
        i = self._bucket_of[id(p)]
        self._pending[i] -= 1
        if self._pending[i] == 0 and self._works[i] is None:
            self._launch(i)
            self.launched_in_backward += 1

    @torch.no_grad()
    def _launch(self, i: int):
        import torch.distributed as dist
        bucket = self.buckets[i]
        if self._flat[i] is None or self._flat[i].device != bucket[0].device:
            self._flat[i] = torch.zeros(sum(p.numel() for p in bucket), dtype=torch.float32, device=bucket[0].device)
            views, off = [], 0
            for p in bucket:
                views.append(self._flat[i][off:off + p.numel()].view_as(p))
                off += p.numel()
            self._views[i] = views
        have = [(v, p.grad) for v, p in zip(self._views[i], bucket) if p.grad is not None and p.grad.data_ptr() != v.data_ptr()]
        for v, p in zip(self._views[i], bucket):
            if p.grad is None:
                v.zero_()
        if have:
            torch._foreach_copy_([v for v, _ in have], [g.to(torch.float32) for _, g in have])
        self._works[i] = dist.all_reduce(self._flat[i], op=dist.ReduceOp.SUM, async_op=True)

    @torch.no_grad()
    def reduce(self):
        import torch.distributed as dist
        if not self._active():
            return
        world = dist.get_world_size()
        for i in range(len(self.buckets)):
            if self._works[i] is None:
                self._launch(i)
        for i, bucket in enumerate(self.buckets):
            self._works[i].wait()
            self._flat[i].div_(world)
            for v, p in zip(self._views[i], bucket):
                p.grad = v if p.dtype == torch.float32 else v.to(p.dtype)
            self._works[i] = None
            self._pending[i] = len(bucket)
