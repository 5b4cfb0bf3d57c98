"""Float64 replay of single inference units, with a bound per output element (tests/test_inference_kernels.py).

A unit is replayed from the GPU's own input to it: the tile, an analysis level (cae_analysis_levels) or a synthesis
bridge.  On the f16x3 path that input is exactly hi + lo of the stored split value, so the host re-splits it with
numpy's round-to-nearest-even float16 conversion (xh = f16(v), xl = f16(v - xh): what the kernels do to a float tile,
and exactly (hi, lo) for a stored value).  Weights and gamma are split the way pack_split does it (csrc/cae_pack.cpp).

Bounds, per element:
  * a convolution whose input the kernel read exactly as given (fp32 path: op(x, w); f16x3: op(xh, wh) + op(xh, wl) +
    op(xl, wh), every f16 product exact in float64): C_CONV * 2^-24 * S, S = op(|x|, |w|) + |b|.  Only the fp32
    accumulation remains, so the bound is as tight on f16x3 as on fp32: a dropped term, a wrong plane, tap or pad fails it;
  * a convolution of a value that was not observed (inside a unit): its input bound through |w|, plus the same
    accumulation term, plus (f16x3) 2^-22 * S for the dropped lo x lo product; the reference uses the split weights;
  * (I)GDN: the bound B_z of the pre-activation through the normalisation to first order,
        GDN   |dy_i| <= B_i / sqrt(N_i) + |z_i| N_i^-3/2 sum_j gamma_ij |z_j| B_j,
        IGDN  |dy_i| <= B_i sqrt(N_i) + |z_i| N_i^-1/2 sum_j gamma_ij |z_j| B_j,
    plus the normalisation's own rounding C_NORM * 2^-22 * |y_i| (f16 squares, rsqrt / sqrt); f16x3 uses the split gamma;
  * LeakyReLU / ReLU are 1-Lipschitz: the bound passes through; a residual sum adds the bounds;
  * a value stored in the split format: + max(2^-22 |v|, 2^-25) (include/cae_hip.h "ACCURACY of f16x3").
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# summation-order constant of every convolution bound.  Largest error / bound observed over tests/test_inference_kernels.py
# on an MI355X: 0.80 on the fp32 path (colour layer, k = 3: 6.4 x 2^-24 S) and 0.40 on f16x3 (last layers, 4 image
# channels and 192 latents); over the walking batches of tests/test_persistent_walk.py (57 samples: more elements to draw
# the maximum from) 0.77 on fp32 and 0.65 on f16x3, both the last layer 40 -> 3 at k = 3; CAE_TEST_VERBOSE=1 prints
# error / bound per result
C_CONV = 8.0
# rounding of the (I)GDN normalisation in units of 2^-22 |y|.  (I)GDN units stay at or below 0.61 of their whole bound
# (fp32 IGDN, 40 and 192 channels), 0.39 on f16x3
C_NORM = 4.0
SPLIT_REL, SPLIT_ABS = 2.0 ** -22, 2.0 ** -25


def split(v: torch.Tensor):
    """(hi, lo) of fp32 values as float64: hi = f16(v), lo = f16(v - hi), both rounded to nearest even"""
    v32 = v.detach().cpu().float()
    hi = v32.half().float()
    lo = (v32 - hi).half()
    return hi.double(), lo.double()


def split_sum(v: torch.Tensor) -> torch.Tensor:
    hi, lo = split(v)
    return hi + lo


def store_split(ref, B):
    """bound of a value after the split store (f16x3): |v - (hi + lo)| <= max(2^-22 |v|, 2^-25)"""
    return B + torch.maximum(SPLIT_REL * (ref.abs() + B), torch.full_like(B, SPLIT_ABS))


# ----------------------------------------------------------------------------------------------------- operators
def op_conv_s2(k):
    P = k // 2
    return lambda x, w: F.conv2d(F.pad(x, (P,) * 4, mode='reflect'), w, stride=2)


def op_conv_s1(k):
    P = k // 2
    return lambda x, w: F.conv2d(F.pad(x, (P,) * 4, mode='reflect'), w)


def op_deconv_s2(k):
    return lambda x, w: F.conv_transpose2d(x, w, stride=2, padding=k // 2, output_padding=1)


def op_deconv_s1(k):
    return lambda x, w: F.conv_transpose2d(x, w, stride=1, padding=k // 2)


def _bias(b, like):
    return 0.0 if b is None else b.detach().cpu().double().view(1, -1, 1, 1).expand_as(like)


def conv_step(op, x, w, b, f16, Bx=None):
    """-> (ref, bound) of one convolution (+ bias).  Bx None: x is exactly what the kernel read (an observed input)."""
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    S = op(x.abs(), w.abs())
    S = S + _bias(b, S).abs() if b is not None else S
    if Bx is None:
        if f16:
            xh, xl = split(x)
            wh, wl = split(w)
            ref = op(xh, wh) + op(xh, wl) + op(xl, wh)
        else:
            ref = op(x, w)
        B = C_CONV * U * S
    else:
        wt = split_sum(w) if f16 else w
        ref = op(x, wt)
        B = op(Bx, wt.abs()) + C_CONV * U * S + (SPLIT_REL * S if f16 else 0.0)
    return ref + _bias(b, ref), B


def gdn_step(z, Bz, beta, gamma, inverse, f16):
    """(I)GDN of the float64 pre-activation z with bound Bz -> (y, By); beta / gamma EFFECTIVE values"""
    g = split_sum(gamma) if f16 else gamma.detach().cpu().double()
    g = g[:, :, None, None]
    beta = beta.detach().cpu().double()
    N = F.conv2d(z * z, g, beta)
    gB = F.conv2d(z.abs() * Bz, g)
    if inverse:
        y = z * torch.sqrt(N)
        By = Bz * torch.sqrt(N) + z.abs() * gB / torch.sqrt(N)
    else:
        y = z / torch.sqrt(N)
        By = Bz / torch.sqrt(N) + z.abs() * gB / N ** 1.5
    return y, By + C_NORM * 2.0 ** -22 * y.abs()


def act_step(v, code):
    return v if code == 0 else (F.leaky_relu(v, 0.01) if code == 1 else F.relu(v))


# ----------------------------------------------------------------------------------------------------- units
def unit_parts(u):
    """(stages, (w, b), gdn (beta, gamma) effective | None, act code) of an analysis / synthesis module unit: exactly
    the tensors _Track._sync uploads"""
    if hasattr(u, 'stages'):
        stages = u.stages()
    elif u.pre is not None:
        pw, pb = u.effective_pre()
        stages = [dict(weight=pw, bias=pb, beta=None, gamma=None, act=u.act_code, add_residual=0, post_act=0)]
    else:
        stages = []
    gdn = u.gdn.effective() if u.gdn is not None else None
    return stages, u.effective_main(), gdn, u.act_code


def _round_ct(c):
    t = (c + 31) // 32
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 6


def stages_need_fp32(cin, stages):
    """csrc/cae_api.hip stages_need_fp32: GDN / residual stages wider than 128 channels run on the fp32 kernels"""
    return _round_ct(cin) > 4 and any(s['beta'] is not None or s['add_residual'] or s['post_act'] for s in stages)


def conv_main_on_fp32(ks, cout, synthesis):
    """csrc/cae_launch_conv_f16.hip conv_f16_fits false: the analysis layer runs on the exact-fp32 kernel (the k = 5,
    192-channel detour); the transposed convolutions always have a split-f16 kernel"""
    if synthesis:
        return False
    ct = _round_ct(cout)
    return 2 * (ks * ct * 2048 + (30 + ks) * 1024) > 160 * 1024


def replay_unit(u, x, ks, synthesis, f16, store_out):
    """unit u applied to the observed input x (float NCHW, what the kernel read) -> (ref, bound) of its output;
    store_out: the output is kept in the split format (f16x3, not the last layer)"""
    stages, (w, b), gdn, act = unit_parts(u)
    x = x.detach().cpu().double()
    cur, B = x, None
    if stages:
        s_f16 = f16 and not stages_need_fp32(x.shape[1], stages)
        op1 = op_deconv_s1(ks) if synthesis else op_conv_s1(ks)
        for sg in stages:
            t, Bt = conv_step(op1, cur, sg['weight'], sg['bias'], s_f16, B)
            if sg['beta'] is not None:
                t, Bt = gdn_step(t, Bt, sg['beta'], sg['gamma'], synthesis, s_f16)
            else:
                t = act_step(t, sg['act'])
            if sg['add_residual']:
                t = t + x  # the unit input as observed: no bound of its own
            cur, B = act_step(t, sg['post_act']), Bt
            if s_f16:
                B = store_split(cur, B)
        if f16 and not s_f16:  # fp32 stages: the last output goes back into the split rows
            B = store_split(cur, B)
    m_f16 = f16 and not conv_main_on_fp32(ks, w.shape[1] if synthesis else w.shape[0], synthesis)
    op = op_deconv_s2(ks) if synthesis else op_conv_s2(ks)
    z, Bz = conv_step(op, cur, w, b, m_f16, B)
    if gdn is not None:
        if m_f16 and _round_ct(z.shape[1]) > 4:  # convolution, split store, then gdn_f16_kernel
            Bz = store_split(z, Bz)
        y, By = gdn_step(z, Bz, gdn[0], gdn[1], synthesis, m_f16)
    else:
        y, By = act_step(z, act), Bz
    if store_out and f16:
        By = store_split(y, By)
    return y, By


# ----------------------------------------------------------------------------------------------------- verdicts
def ratio(got, ref, bound):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


def judge(got, ref, bound, what):
    r = ratio(got, ref, bound)
    if os.environ.get('CAE_TEST_VERBOSE'):
        err = float((got.detach().cpu().double() - ref).abs().max())
        print(f'{what}: err / bound {r:.3f}, max err {err:.2e}, max |ref| {float(ref.abs().max()):.2e}')
    assert r <= 1.0, (what, r)
    return r


def judge_u8(got_u8, ref, bound, what):
    """u8 == trunc(clip(255 ref)) except where 255 ref lies within 255 bound of an integer (then either neighbour)"""
    v = 255.0 * ref
    e = 255.0 * bound + 1e-9
    lo = torch.floor((v - e).clamp(0, 255))
    hi = torch.floor((v + e).clamp(0, 255))
    got = got_u8.detach().cpu().double()
    bad = (got < lo) | (got > hi)
    if os.environ.get('CAE_TEST_VERBOSE'):
        print(f'{what}: {int(bad.sum())} of {got.numel()} u8 values outside trunc(clip(255 ref +- 255 bound))')
    assert not bool(bad.any()), (what, int(bad.sum()))
