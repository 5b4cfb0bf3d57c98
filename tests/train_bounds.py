"""Float64 references and first-order error bounds of the fused GDN and density training kernels, and float32 emulations
of the kernels' arithmetic (tests/test_train_gdn_density.py).

Conventions: u = 2^-24 (the unit roundoff of fp32); an fp32 operation contributes C * u * sum|terms| (a sum) or u * |result|
(one rounding); an input carries the error it already has, passed on to first order.  Bounds are absolute, per element.

GDN / IGDN (include/cae_hip.h, csrc/cae_train_gdn.hpp), with e = -1/2 (GDN) or +1/2 (IGDN), on channels-last [pixels][c]:
    n = beta + z^2 Gamma^T            all terms >= 0: relative error (C_SUM + c / 2) u
    f = n^e,  y = z f                 relative error half of that + ULP_RSQ ulp + one rounding
    g = fold(g_ext)                   the reflect fold (F.pad's backward), <= 4 fp32 terms: 3 u sum|terms|
    g_n = g e z n^(e-1)               relative error |e - 1| times n's + the rsq / rcp / sqrt ulps and four roundings
    t = g_n Gamma,  g_z = g f + 2 z t          sum|terms| bounds, plus the errors g_n and g carry
    g_Gamma = g_n^T z^2,  g_beta = sum g_n     sum|terms| bounds, plus the errors g_n carries
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# summation-order constant of every fp32 sum.  Worst error / bound observed on an MI355X over
# tests/test_train_gdn_density.py (CAE_TEST_VERBOSE=1 prints each): GDN y32 0.36, g_z (fp32) 0.28, g_Gamma 0.20,
# g_beta 0.12, bf16 outputs 0.50 (their rounding); density lik 0.14, g_y 0.99 (its last rounding), raw-parameter
# gradients 0.005; reparam 0.50; clip + Adam 0.97 (param), 0.85 (exp_avg), 0.92 (exp_avg_sq) -- the last roundings
C_SUM = 8.0
# accuracy of the gfx950 v_rsq_f32 / v_sqrt_f32 / v_rcp_f32 instructions used by the GDN kernels, in ulp (1 ulp <= 2u
# relative): documented as 1 ulp; 1 is what the bound uses
ULP_RSQ = 1.0


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp of each value (8 significant bits; the smallest normal's ulp below it)"""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def ratio(got, ref, bound) -> float:
    """max over elements of |got - ref| / bound (0 / 0 = 0); inf where got is not finite"""
    got, ref, bound = got.double(), ref.double(), bound.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def report(what, r):
    if os.environ.get('CAE_TEST_VERBOSE'):
        print(f'{what}: max err / bound {r:.3f}')


def judge(got, ref, bound, what):
    r = ratio(got, ref, bound)
    report(what, r)
    assert r <= 1.0, (what, r)
    return r


# ---------------------------------------------------------------------------------------------------------------- GDN
def fold(gext, n, h, w, pad):
    """reflect fold of an extended-domain gradient, channels-last [n][h + 2 pad][w + 2 pad][c] -> [n h w][c] (float64)"""
    c = gext.shape[-1]
    g = gext.double().reshape(n, h + 2 * pad, w + 2 * pad, c).permute(0, 3, 1, 2)
    if pad == 0:
        return g.permute(0, 2, 3, 1).reshape(-1, c)
    x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    F.pad(x, (pad,) * 4, mode='reflect').backward(g)
    return x.grad.permute(0, 2, 3, 1).reshape(-1, c)


def gdn_reference(z, beta, gamma, inverse, gext=None, shape=None, pad=0):
    """float64 GDN / IGDN on fp32 operands (z [pixels][c], beta [c], gamma [c][c]; gext the extended-domain gradient
    [n][h + 2 pad][w + 2 pad][c], shape = (n, h, w)) -> dict of reference values and their bounds B_*"""
    z, beta, gamma = z.double(), beta.double(), gamma.double()
    e = 0.5 if inverse else -0.5
    z2 = z * z
    nrm = beta + z2 @ gamma.t()
    f = nrm ** e
    y = z * f
    # relative error of n: every term is >= 0, so each of the ~c / 2 sequential MFMA k-steps rounds by at most u of n
    # (the error grows with the depth: 7.1 u n at c = 192 on an MI355X, beyond C_SUM alone)
    eps_n = (C_SUM + z.shape[1] / 2) * U
    rel_f = 0.5 * eps_n + 2 * ULP_RSQ * U
    out = dict(y=y, B_y=(rel_f + U) * y.abs())
    if gext is None:
        return out
    n, h, w = shape
    g, gabs = fold(gext, n, h, w, pad), fold(gext.abs(), n, h, w, pad)
    Eg = 3 * U * gabs
    a = e * z * nrm ** (e - 1)
    rel_a = abs(e - 1) * eps_n + (2 * 2 * ULP_RSQ + 4) * U  # rsq^3 (or rcp of sqrt) + four roundings
    gn = g * a
    Egn = a.abs() * Eg + gn.abs() * rel_a
    gzd = g * f
    Egzd = f * Eg + gzd.abs() * (rel_f + U)
    ga = gamma.abs()
    t = gn @ gamma
    St = gn.abs() @ ga
    Et = Egn @ ga + C_SUM * U * St
    gz = gzd + 2 * z * t
    Bgz = Egzd + 2 * z.abs() * Et + 2 * U * (gzd.abs() + 2 * (z * t).abs())
    ggamma = gn.t() @ z2
    Bgg = Egn.t() @ z2 + (C_SUM + 2) * U * (gn.abs().t() @ z2)
    gbeta = gn.sum(0)
    Bgb = Egn.sum(0) + C_SUM * U * gn.abs().sum(0)
    out.update(g=g, gn=gn, gz=gz, B_gz=Bgz, ggamma=ggamma, B_ggamma=Bgg, gbeta=gbeta, B_gbeta=Bgb)
    return out


def _fold_f32(gext, n, h, w, pad, mutate=None):
    """fold_inplace_kernel in float32: every interior pixel next to the border adds its mirror images in the ring"""
    ge = gext.float().reshape(n, h + 2 * pad, w + 2 * pad, -1)
    g = ge[:, pad:pad + h, pad:pad + w].clone()
    if pad == 0:
        return g.reshape(n * h * w, -1)

    def mirrors(y, H):
        m = [y]
        if 1 <= y <= pad:
            m.append(-y)
        if H - 1 - pad <= y <= H - 2:
            m.append(2 * (H - 1) - y)
        return m
    for y in range(h):
        ys = mirrors(y, h)
        if mutate == 'fold_skips_row0' and y == 0 and h <= pad + 1:
            ys = [0]
        for x in range(w):
            xs = mirrors(x, w)
            if len(ys) * len(xs) == 1:
                continue
            s = torch.zeros_like(g[:, 0, 0])
            for yy in ys:
                for xx in xs:
                    s = s + ge[:, yy + pad, xx + pad]
            g[:, y, x] = s
    return g.reshape(n * h * w, -1)


def _blocked_sum(terms, seed, dim):
    """float32 sum over `dim` in a shuffled order, 16-term fp32 partial sums added sequentially"""
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(terms.shape[dim]))
    terms = terms.index_select(dim, perm)
    acc = None
    for s in range(0, terms.shape[dim], 16):
        part = terms.narrow(dim, s, min(16, terms.shape[dim] - s)).sum(dim, dtype=torch.float32)
        acc = part if acc is None else acc + part
    return acc


def emulate_gdn(z, beta, gamma, inverse, gext, shape, pad, seed, mutate=None):
    """the fused GDN pair in float32 (32-pixel tiles, the last one ragged and clamped; per-tile sums) -> y, g_z, g_Gamma,
    g_beta as float64.  `mutate` plants one defect."""
    n, h, w = shape
    z, beta, gamma = z.float(), beta.float(), gamma.float()
    P, c = z.shape
    T = (P + 31) // 32
    idx = torch.clamp(torch.arange(T * 32), max=P - 1)  # clamped rows of the last tile
    zt = z[idx]
    z2 = zt * zt
    nrm = beta + _blocked_sum(z2[:, None, :] * gamma[None], seed, 2)
    f = torch.sqrt(nrm) if inverse else 1.0 / torch.sqrt(nrm)
    y = (zt * f)[:P]
    g = _fold_f32(gext, n, h, w, pad, mutate)[idx]
    fb = f
    if mutate == 'last_tile_reads_previous_f' and T >= 2:
        fb = f.clone()
        fb[(T - 1) * 32:] = f[(T - 2) * 32:(T - 1) * 32]
    valid = (torch.arange(T * 32) < P).float()[:, None]
    if mutate == 'clamped_rows_in_ggamma':
        valid = torch.ones_like(valid)
    gn = (0.5 * g * zt / fb) if inverse else (-0.5 * g * zt * fb * fb * fb)
    gn = gn * valid
    gzd = g * fb
    G = gamma.t() if mutate == 'gamma_for_gamma_t' else gamma
    t = _blocked_sum(gn[:, :, None] * G[None], seed + 1, 1)  # t[p][j] = sum_c gn[p][c] G[c][j]
    cross = 2.0 * zt * t
    if mutate == 'drop_cross_term_on_tile_1':
        cross[:, 32:64] = 0.0
    gz = (gzd + cross)[:P]
    # parameter gradients: per-tile fp32 partial sums, then the tiles in order (the flush)
    ggp = torch.einsum('tpc,tpj->tcj', gn.reshape(T, 32, c), z2.reshape(T, 32, c))
    ggamma = _blocked_sum(ggp, seed + 2, 0)
    gbeta = _blocked_sum(gn.reshape(T, 32, c).sum(1), seed + 3, 0)
    return y.double(), gz.double(), ggamma.double(), gbeta.double()


# ---------------------------------------------------------------------------------------- first-order error arithmetic
# Accuracy of the device library's elementary functions on gfx950, in ulp (1 ulp <= 2u relative).  The library's own
# accuracy table is not shipped with ROCm; the corresponding CUDA functions are documented at <= 2 ulp (expf, tanhf) and
# 1 ulp (log1pf).  The bound takes 4 ulp for each, a margin of 2x over those documented figures; on the MI355X the
# density outputs stay at or below 0.14 (lik) and 0.005 (raw-parameter gradients) of their bounds.
ULP_EXP = ULP_LOG1P = ULP_TANH = 4.0
TINY = 2.0 ** -148  # absolute floor of one rounding (subnormal results)


class EV:
    """a float64 value with an absolute first-order bound on the error of its fp32 evaluation"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    def __neg__(self):
        return EV(-self.v, self.e)


def _ev(x):
    return x if isinstance(x, EV) else EV(torch.as_tensor(x, dtype=torch.float64))


def _rnd(v):
    return U * v.abs() + TINY


class EVA:
    """operations of EV numbers: every result rounds once"""

    @staticmethod
    def add(a, b):
        a, b = _ev(a), _ev(b)
        v = a.v + b.v
        return EV(v, a.e + b.e + _rnd(v))

    @staticmethod
    def sub(a, b):
        return EVA.add(a, -_ev(b))

    @staticmethod
    def mul(a, b):
        a, b = _ev(a), _ev(b)
        v = a.v * b.v
        return EV(v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + _rnd(v))

    @staticmethod
    def fma(a, b, c):  # (two roundings: covers a contracted and an uncontracted evaluation)
        a, b, c = _ev(a), _ev(b), _ev(c)
        p = a.v * b.v
        v = p + c.v
        return EV(v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + c.e + _rnd(p) + _rnd(v))

    @staticmethod
    def tanh(a):
        a = _ev(a)
        v = torch.tanh(a.v)
        slope = 1 - torch.tanh((a.v.abs() - a.e).clamp_min(0)) ** 2  # the largest slope within the error interval
        return EV(v, slope * a.e + ULP_TANH * 2 * U * v.abs() + TINY)

    @staticmethod
    def sigmoid(a):
        """1 / (1 + expf(-x)): expf's ulps, the add and the division; expf(-x) overflows below x = -88 (result 0)"""
        a = _ev(a)
        v = torch.sigmoid(a.v)
        xm = (a.v.abs() - a.e).clamp_min(0)
        slope = torch.sigmoid(xm) * torch.sigmoid(-xm)
        e = slope * a.e + (2 * ULP_EXP + 2) * U * v + TINY
        return EV(v, e + torch.where(a.v < -80, v, torch.zeros_like(v)))

    @staticmethod
    def softplus(r):
        """x > 20 ? x : log1pf(expf(x)) of an exact fp32 value"""
        r = torch.as_tensor(r, dtype=torch.float64)
        E = torch.exp(r.clamp_max(20))
        v = torch.where(r > 20, r, torch.log1p(E))
        e = ULP_EXP * 2 * U * E / (1 + E) + ULP_LOG1P * 2 * U * v + TINY
        return EV(v, torch.where(r > 20, torch.zeros_like(v), e))

    @staticmethod
    def sqrt(a):
        a = _ev(a)
        v = torch.sqrt(a.v)
        return EV(v, a.e / (2 * v) + 2 * ULP_RSQ * U * v + TINY)

    @staticmethod
    def div(a, b):
        a, b = _ev(a), _ev(b)
        v = a.v / b.v
        return EV(v, (a.e + v.abs() * b.e) / b.v.abs() + _rnd(v))


class F32A:
    """the same operations on float32 tensors (CPU emulation of the kernels' arithmetic)"""
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    mul = staticmethod(lambda a, b: a * b)
    fma = staticmethod(lambda a, b, c: a * b + c)
    tanh = staticmethod(torch.tanh)
    sigmoid = staticmethod(lambda x: 1.0 / (1.0 + torch.exp(-x)))

    @staticmethod
    def softplus(r, threshold=20.0):
        r = torch.as_tensor(r, dtype=torch.float32)
        return torch.where(r > threshold, r, torch.log1p(torch.exp(r)))


# ------------------------------------------------------------------------------------------------------------ density
D, K = 3, 4  # filters (3, 3, 3, 3): the built shape
DIN = [1, D, D, D, D]
DOUT = [D, D, D, D, 1]
M_OFF = [0, D, D + D * D, D + 2 * D * D, D + 3 * D * D]
NM = D + (K - 1) * D * D + D
B_OFF = [NM + i * D for i in range(K + 1)]
NB = K * D + 1
F_OFF = [NM + NB + i * D for i in range(K)]
NP = NM + NB + K * D


def transformed(A, raw, threshold=20.0):
    """raw (C, NP) -> {'M': [i][j][k], 'b': [i][j], 'F': [i][j]} of (C, 1) numbers: softplus | bias | tanh"""
    col = lambda i: raw[:, i:i + 1]  # noqa: E731
    ev = A is EVA
    sp = A.softplus if ev else (lambda r: A.softplus(r, threshold))
    M = [[[sp(col(M_OFF[i] + j * DIN[i] + k)) for k in range(DIN[i])] for j in range(DOUT[i])] for i in range(K + 1)]
    b = [[(EV(col(B_OFF[i] + j).double()) if ev else col(B_OFF[i] + j)) for j in range(DOUT[i])] for i in range(K + 1)]
    Fa = [[A.tanh(col(F_OFF[i] + j)) for j in range(D)] for i in range(K)]
    return dict(M=M, b=b, F=Fa)


def logits(A, T, x):
    """the kernel's logits(): fmaf chains, tanh, out = fmaf(factor, t, z) -> (logit, inputs of every layer, tanh values)"""
    h, hs, ts = [x], [], []
    z0 = None
    for i in range(K + 1):
        hs.append(h)
        outs, tl = [], []
        for j in range(DOUT[i]):
            z = T['b'][i][j]
            for k in range(DIN[i]):
                z = A.fma(T['M'][i][j][k], h[k], z)
            if i < K:
                t = A.tanh(z)
                tl.append(t)
                outs.append(A.fma(T['F'][i][j], t, z))
            else:
                z0 = z
        if i < K:
            ts.append(tl)
            h = outs
    return z0, hs, ts


def backprop(A, gl, T, hs, ts, acc, mutate=None):
    """the kernel's backprop(): parameter gradients (w.r.t. the TRANSFORMED parameters) into acc.add(index, value);
    -> d loss / d input"""
    acc.add(B_OFF[K], gl)
    dout = []
    for k in range(D):
        acc.add(M_OFF[K] + k, A.mul(gl, hs[K][k]))
        dout.append(A.mul(T['M'][K][0][k], gl))
    for i in range(K - 1, -1, -1):
        dz = []
        for j in range(D):
            t = ts[i][j]
            acc.add(F_OFF[i] + j, A.mul(dout[j], t))
            one_m = A.sub(1.0, t) if mutate == 'one_minus_t' else A.sub(1.0, A.mul(t, t))
            dz.append(A.mul(dout[j], A.fma(T['F'][i][j], one_m, 1.0)))
            acc.add(B_OFF[i] + j, dz[j])
        din = []
        for k in range(DIN[i]):
            s = 0.0
            for j in range(D):
                acc.add(M_OFF[i] + j * DIN[i] + k, A.mul(dz[j], hs[i][k]))
                s = A.fma(T['M'][i][j][k], dz[j], s)
            din.append(s)
        dout = din
    return dout[0]


# Worst-case depth of the kernels' fp32 reduction of a parameter gradient, in units of u * sum|terms|: a thread's
# sequential sum over <= 9 elements x 2 evaluations, the 6-step wave shuffle, the 4 waves, the chain rule and <= 32 atomics
C_RED = 64.0


class _EVAcc:
    """sum over the elements of every parameter's contributions: value (primary weight w), its error, sum|terms| and the
    allowance of elements whose branch the kernel may take either way (weight amb)"""

    def __init__(self, C, w, amb):
        z = lambda: torch.zeros(NP, C, dtype=torch.float64)  # noqa: E731
        self.val, self.err, self.abs, self.allow = z(), z(), z(), z()
        self.w, self.amb = w, amb
        self.any = (w > 0) | (amb > 0)

    def add(self, i, x):
        self.val[i] += (self.w * x.v).sum(1)
        self.err[i] += (self.any * x.e).sum(1)
        self.abs[i] += (self.any * x.v.abs()).sum(1)
        self.allow[i] += (self.amb * x.v.abs()).sum(1)


def density_reference(raw, v, g_lik=None, g_out=None, plain=True, bound=1e-9):
    """float64 density of one kernel call on v = out (C, E) (fp32 values; rows = channels), raw (C, NP) fp32, with
    first-order bounds.  -> dict(lik, B_lik[, g_y, B_gy, g_raw, B_graw])"""
    raw64 = raw.double()
    A = EVA
    T = transformed(A, raw64)
    v = v.double()
    xs = [EV(v + d, _rnd(v + d)) for d in (-0.5, 0.5)]  # (v -+ 0.5f rounds once)
    (lo, hl, tl), (up, hu, tu) = logits(A, T, xs[0]), logits(A, T, xs[1])
    one = lambda: torch.ones_like(v)  # noqa: E731
    zero = torch.zeros_like(v)
    if plain:
        su, sl = A.sigmoid(up), A.sigmoid(lo)
        p = A.sub(su, sl)
        dpu, dpl = A.mul(su, A.sub(1.0, su)), -A.mul(sl, A.sub(1.0, sl))
        ws, a1, a3 = one(), zero, zero
    else:
        ssum = A.add(lo, up)
        a1 = (ssum.v.abs() <= ssum.e).double()  # the kernel's sign may differ (+-1, or 0)
        ws = (ssum.v != 0).double()  # sign(0) = 0: p = 0, no gradient from the likelihood

        def branch(s):
            su, sl = A.sigmoid(EV(s * up.v, up.e)), A.sigmoid(EV(s * lo.v, lo.e))
            q = A.sub(su, sl)
            sq = torch.sign(q.v)
            return q, A.mul(su, A.sub(1.0, su)), A.mul(sl, A.sub(1.0, sl)), sq * s
        s = torch.where(ssum.v >= 0, -one(), one())
        q, du, dl, k = branch(s)
        q2, du2, dl2, _ = branch(-s)
        mx = lambda x, y: EV(x.v, torch.where(a1 > 0, torch.maximum(x.e, y.e), x.e))  # noqa: E731
        q, du, dl = mx(q, q2), mx(du, du2), mx(dl, dl2)
        a3 = (q.v.abs() <= q.e).double()  # sign(q) may differ
        p = EV(q.v.abs(), q.e)
        dpu, dpl = EV(k * du.v, du.e), EV(-k * dl.v, dl.e)
    pref = ws * p.v
    lik = pref.clamp_min(bound)
    out = dict(lik=lik, B_lik=p.e + a1 * (p.v.clamp_min(bound) - bound), p=pref, B_p=p.e)
    if g_lik is None:
        return out
    g_lik = g_lik.double()
    passes = ((pref >= bound) | (g_lik < 0)).double()
    a2 = ((p.v - bound).abs() <= p.e).double() * (g_lik >= 0).double()
    w = passes * ws
    amb = a1 + a2 + 2 * a3
    acc = _EVAcc(v.shape[0], w, amb)
    gu, gl = A.mul(g_lik, dpu), A.mul(g_lik, dpl)
    gv = A.add(backprop(A, gu, T, hu, tu, acc), backprop(A, gl, T, hl, tl, acc))
    go = zero if g_out is None else g_out.double()
    gy = w * gv.v + go
    any_ = ((w > 0) | (amb > 0)).double()
    B_gy = any_ * gv.e + amb * gv.v.abs() + _rnd(gy)
    # chain rule to the raw parameters: d softplus = r > 20 ? 1 : sigmoid(r) (fp32 expf), d tanh = 1 - tanh^2
    S = acc.val.t()
    BS = (acc.err + C_RED * U * acc.abs + acc.allow).t()
    absS = acc.abs.t()
    d = torch.ones_like(raw64)
    Ed = torch.zeros_like(raw64)
    rm = raw64[:, :NM]
    sg = A.sigmoid(rm)
    d[:, :NM] = torch.where(rm > 20, torch.ones_like(rm), sg.v)
    Ed[:, :NM] = torch.where(rm > 20, torch.zeros_like(rm), sg.e)
    tf = A.tanh(raw64[:, NM + NB:])
    dt = A.sub(1.0, A.mul(tf, tf))
    d[:, NM + NB:], Ed[:, NM + NB:] = dt.v, dt.e
    g_raw = S * d
    B_graw = BS * d.abs() + (absS + BS) * Ed + U * (absS * d.abs()) + TINY
    out.update(g_y=gy, B_gy=B_gy, g_raw=g_raw, B_graw=B_graw)
    return out


def emulate_density(raw, v, g_lik, g_out, plain, bound, seed, mutate=None):
    """cae_t_density_forward / backward in float32 on the CPU (rows = channels; grid of blocks_per_channel blocks of 256
    threads walking the elements, per-thread accumulation, then the blocks' partial sums in a shuffled order)
    -> lik, g_y, g_raw as float64.  `mutate` plants one defect."""
    A = F32A
    C, E = v.shape
    T = transformed(A, raw.float(), threshold=4.0 if mutate == 'softplus_threshold_4' else 20.0)
    v = v.float()
    lo, hl, tl = logits(A, T, v - 0.5)
    up, hu, tu = logits(A, T, v + 0.5)
    if plain:
        su, sl = A.sigmoid(up), A.sigmoid(lo)
        p = su - sl
        dpu, dpl = su * (1 - su), -sl * (1 - sl)
    else:
        s = -torch.sign(lo + up)
        su, sl = A.sigmoid(s * up), A.sigmoid(s * lo)
        q = su - sl
        sq = torch.sign(q)
        p = q.abs()
        dpu, dpl = sq * s * su * (1 - su), -sq * s * sl * (1 - sl)
    lik = torch.clamp_min(p, bound)
    passes = (p >= bound) | (g_lik < 0)
    if mutate == 'lowerbound_inverted':
        passes = ~passes
    gp = torch.where(passes, g_lik.float(), torch.zeros_like(p))
    blocks = min(max((E + 2047) // 2048, 1), 32)
    stride = blocks * 256
    keep = torch.ones(E)
    if mutate == 'drop_last_loop_round':
        keep[(E - 1) // stride * stride:] = 0.0
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(stride))

    class Acc:
        def __init__(self):
            self.g = torch.zeros(NP, C)

        def add(self, i, x):  # per-thread fp32 sums over the loop rounds, then the threads in a shuffled order
            x = torch.broadcast_to(x, (C, E)) * keep
            pad = (-E) % stride
            xt = torch.cat([x, torch.zeros(C, pad)], 1).reshape(C, -1, stride)
            per_thread = xt[:, 0]
            for r in range(1, xt.shape[1]):
                per_thread = per_thread + xt[:, r]
            self.g[i] += _blocked_sum(per_thread[:, perm], seed, 1)
    acc = Acc()
    gv = backprop(A, gp * dpu, T, hu, tu, acc, mutate) + backprop(A, gp * dpl, T, hl, tl, acc, mutate)
    gy = gv + (0.0 if g_out is None else g_out.float())
    rf = raw.float()
    d = torch.ones_like(rf)
    thr = 4.0 if mutate == 'softplus_threshold_4' else 20.0
    d[:, :NM] = torch.where(rf[:, :NM] > thr, torch.ones_like(rf[:, :NM]), A.sigmoid(rf[:, :NM]))
    tf = torch.tanh(rf[:, NM + NB:])
    d[:, NM + NB:] = 1 - tf * tf
    g_raw = acc.g.t() * d
    return lik.double(), gy.double(), g_raw.double()


class F64A(F32A):
    """plain float64 evaluation (no error tracking): input search"""

    @staticmethod
    def softplus(r, threshold=20.0):
        r = torch.as_tensor(r, dtype=torch.float64)
        return torch.where(r > threshold, r, torch.log1p(torch.exp(r.clamp_max(threshold))))


def density_p(raw, v, plain=True):
    """float64 p(v) of every channel (rows), as the reference defines it (sign(0) = 0)"""
    A = F64A
    T = transformed(A, raw.double())
    v = v.double()
    lo, up = logits(A, T, v - 0.5)[0], logits(A, T, v + 0.5)[0]
    if plain:
        return torch.sigmoid(up) - torch.sigmoid(lo)
    s = -torch.sign(lo + up)
    return (torch.sigmoid(s * up) - torch.sigmoid(s * lo)).abs()


def density_autograd(raw, v, g_lik, g_out, plain, bound):
    """float64 autograd of oracle.train_oracle.entropy_forward (LowerBound rule included) on float64 copies of the raw
    parameters -> (g_y, g_raw (C, NP))"""
    from oracle import train_oracle as TO
    C = raw.shape[0]
    raw64 = raw.double().clone().requires_grad_(True)
    params = {}
    for i in range(K + 1):
        params[f'_matrix{i}'] = raw64[:, M_OFF[i]:M_OFF[i] + DOUT[i] * DIN[i]].reshape(C, DOUT[i], DIN[i])
        params[f'_bias{i}'] = raw64[:, B_OFF[i]:B_OFF[i] + DOUT[i]].reshape(C, DOUT[i], 1)
        if i < K:
            params[f'_factor{i}'] = raw64[:, F_OFF[i]:F_OFF[i] + D].reshape(C, D, 1)
    y = v.double()[None].clone().requires_grad_(True)
    _, lik = TO.entropy_forward(params, y, None, K, form='plain' if plain else 'sign', bound=bound)
    (lik[0] * g_lik.double()).sum().backward()
    gy = y.grad[0] + (0.0 if g_out is None else g_out.double())
    return gy, raw64.grad
