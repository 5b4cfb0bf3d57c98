"""f16x3 range guard, store site by store site (include/cae_hip.h, "VALID RANGE of f16x3").

tests/test_range_guard.py shows that the guard exists: its overflow cases scale a whole layer, so thousands of values
overflow in every lane, channel tile and sample.  Here every case makes ONE value unstorable (|v| = 1.1 x 65504), at a
chosen tensor, channel, sample and pixel, so that a store site whose maximum skipped a lane, a channel tile, a ragged
edge or a sample would return wrong results without a fallback.  The sites (cnn_autoencoder_amd/csrc/cae_kernels_f16.hpp):
store_split_f16 behind conv_first_f16_kernel, conv_s2_f16_kernel (S = 2; S = 1 reflect, zero padding, residual sum) and
deconv_s2_f16_kernel; store_pmap_f16; gdn_f16_kernel (192 channels: the pre-GDN store of the convolution and the
post-IGDN store); nchw_to_c8s_kernel<SP> with and without the fused dequantiser; c8_to_c8s_kernel<SP> behind the fp32
stages of units wider than 128 channels; the scaled decode.

How one value is made large and everything else stays small (float64 replay of the track, `_replay`):
  * analysis: dark tiles rng.integers(0, 12) with one 2 x 2 patch of 255 below the target pixel; synthesis: small
    latents with one hot latent pixel.  The window the target pixel reads then has the largest energy of its layer;
  * output channel c of the layer that writes the target is a MATCHED FILTER: its weights are that window (the gradient
    of the target element with respect to the weights, so padding and the sub-pixel phases of the transposed
    convolution need no index arithmetic), times s.  By Cauchy-Schwarz the response is largest at the target; for a
    transposed convolution the taps of the other three output parities are zero, so they hold 0 in channel c;
  * a (I)GDN behind it lets channel c through: row and column c of the effective gamma are zero, beta_c = 1;
  * every consumer reads channel c with ZERO weights.  (The issue's 1 / s would do on the oracle, but not on the device
    within the project's 1e-4: a weight below 2^-3 is stored to 2^-25 absolute, times 6e4 that is 2e-3 per tap.)
  * s is found by iterating s *= wanted / value (one step where the map is linear).
The twin of a case has the same value at 0.9 x 65504: nothing may raise, and the f16x3 result itself is judged.

CPU tests check the table: the premise (exactly one stored element above 65504, where the case says, every other below
0.9 x 65504), the sensitivity (the target rounded through the split format gives a non-finite result) and the twin.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import inference_replay as R
from conftest import oracle_layers
from test_range_guard import RTOL, _close

F16_MAX = 65504.0
OVER, UNDER = 1.1, 0.9


# ----------------------------------------------------------------------------------------------------- models
def _track(kind, seed, kw):
    """Analyzer ('enc') / Synthesizer ('dec') of synth.CANONICAL + kw with synth.synthetic_state's parameters (residual and
    multiscale models, which synthetic_state does not describe: the seeded weights of tests/test_inference_kernels.py)"""
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import synth
    cfg = dict(synth.CANONICAL, **kw)
    torch.manual_seed(seed)
    mod = (cae.Analyzer if kind == 'enc' else cae.Synthesizer)(**cfg)
    if cfg['use_residual'] or cfg.get('multiscale_analysis'):
        from test_inference_kernels import _realistic
        _realistic(mod, seed)
    else:
        state = synth.synthetic_state(cfg, seed=seed)
        res = mod.load_state_dict(state['encoder' if kind == 'enc' else 'decoder'], strict=False)
        assert not res.unexpected_keys and all('weight' not in k and k.split('.')[-1] not in ('beta', 'gamma', 'bias')
                                               for k in res.missing_keys), res
    return mod.eval(), cfg


def _stage_conv(u, k=0):
    return u.res_model[u._res[k][0]] if hasattr(u, '_res') else u.pre


def _stage_gdn(u, k=0):
    gi = u._res[k][2] if hasattr(u, '_res') else None
    return None if gi is None else u.res_model[gi]


def _out_channel(conv, c):
    return conv.weight.data[:, c] if conv.transposed else conv.weight.data[c]


def _in_channel(conv, c):
    return conv.weight.data[c] if conv.transposed else conv.weight.data[:, c]


def _let_through(gdn, c, beta=1.0):
    """channel c of a (I)GDN: norm_c = beta, and no other channel's norm sees it"""
    from oracle import cae_oracle as O
    be, ga = (t.clone() for t in gdn.effective())
    be[c] = beta
    ga[c, :] = 0.0
    ga[:, c] = 0.0
    gdn.beta.data.copy_(O.nonneg_init(be))
    gdn.gamma.data.copy_(O.nonneg_init(ga))


# ----------------------------------------------------------------------------------------------------- float64 replay
def _gdn(z, gdn, inverse):
    beta, gamma = (t.detach().double() for t in gdn)
    n = torch.nn.functional.conv2d(z * z, gamma[:, :, None, None], beta)
    return z * torch.sqrt(n) if inverse else z / torch.sqrt(n)


def _conv(op, x, w, b):
    y = op(x, w.detach().double())
    return y if b is None else y + b.detach().double().view(1, -1, 1, 1)


def _replay(track, x, synthesis, nrun=None, hook=None, probe=None):
    """The call in float64 on the tensors _Track._sync uploads.  hook(name, tensor) -> tensor is called for every tensor
    the f16x3 route of csrc/cae_api.hip writes in the split format, in order ('input': the layout conversion, absent
    when the first analysis layer reads the tile itself; 'u{i}.s{k}': stride-1 stage k of unit i; 'u{i}.stages': the
    last stage of a unit whose stages run on the fp32 kernels; 'u{i}.pre': the convolution of a GDN unit wider than 128
    channels; 'u{i}.out': the unit; the last unit writes fp32 or uint8).  probe[name + '.in']: what the convolution that
    writes `name` read.  nrun < L: the scaled decode, units 0 .. nrun-1 and colour layer nrun-1."""
    hook = hook or (lambda name, t: t)
    probe = {} if probe is None else probe
    ks, units = track._dims[4], track._units()
    L = len(units)
    nrun = L if nrun is None else nrun
    s1 = R.op_deconv_s1(ks) if synthesis else R.op_conv_s1(ks)
    s2 = R.op_deconv_s2(ks) if synthesis else R.op_conv_s2(ks)
    cur = x.double()
    if synthesis or track._dims[0] > 4 or R.unit_parts(units[0])[0]:
        cur = hook('input', cur)
    for i, u in enumerate(units[:nrun]):
        stages, (w, b), gdn, act = R.unit_parts(u)
        unit_in = cur
        on_fp32 = R.stages_need_fp32(cur.shape[1], stages)
        for k, sg in enumerate(stages):
            probe[f'u{i}.s{k}.in'] = cur
            t = _conv(s1, cur, sg['weight'], sg['bias'])
            t = _gdn(t, (sg['beta'], sg['gamma']), synthesis) if sg['beta'] is not None else R.act_step(t, sg['act'])
            if sg['add_residual']:
                t = t + unit_in
            cur = R.act_step(t, sg['post_act'])
            if not on_fp32:
                cur = hook(f'u{i}.s{k}', cur)
        if stages and on_fp32:
            cur = hook(f'u{i}.stages', cur)
        probe[f'u{i}.out.in'] = cur
        z = _conv(s2, cur, w, b)
        last = i == L - 1
        if gdn is not None:
            assert not R.conv_main_on_fp32(ks, z.shape[1], synthesis)  # (the k = 5, 192-channel detour is not in the table)
            if not last and R._round_ct(z.shape[1]) > 4:
                z = hook(f'u{i}.pre', z)
            y = _gdn(z, gdn, synthesis)
        else:
            y = R.act_step(z, act)
        cur = y if last else hook(f'u{i}.out', y)
    if nrun < L:
        conv = track.color_layers[nrun - 1][0]
        cur = _conv(R.op_conv_s1(ks), cur, conv.dense_weight(), conv.bias)
    return cur


# ----------------------------------------------------------------------------------------------------- the case table
# name: (kind, track kwargs, input shape, entry, target tensor, channel, (sample, y, x) -- negative: from the end, extras)
#   kind 'conv':   the convolution that writes the target carries the matched filter in channel c
#        'res':    the target is a residual sum x_c + g x_c of two storable addends: the matched filter sits in the unit
#                  before (x_c = 0.6 x 65504 at 1.1), the stage's channel c is g = 5/6 times the centre tap of channel c
#        'spike':  one element of the input / the latents
# input shape: analysis (n, h, w) tiles, synthesis (n, lh, lw) latents.
GDN32 = dict(channels_net=32, channels_bn=48, compression_level=3)
GDN40 = dict(channels_net=40, channels_bn=48, compression_level=3)
NONE40 = dict(GDN40, act_layer_type=None)
LRELU40 = dict(GDN40, act_layer_type='LeakyReLU')
RES40 = dict(GDN40, use_residual=True)
GDN192 = dict(channels_net=192, channels_bn=48, compression_level=3)
C8 = dict(channels_org=8, channels_net=40, channels_bn=48, compression_level=2)
RES160_ENC = dict(channels_net=160, channels_bn=16, compression_level=3, use_residual=True)
RES160_DEC = dict(channels_net=160, channels_bn=160, compression_level=2, use_residual=True)
LAT2 = dict(channels_net=40, channels_bn=48, compression_level=2)
MULTI32 = dict(channels_net=32, channels_bn=16, compression_level=4, multiscale_analysis=True)
FIRST, LAST = (0, 0, 0), (-1, -1, -1)

CASES = {
    # conv_first_f16_kernel: 37 x 70 tiles -> 19 x 35 (16 x 16 tiles: 3 rows and 3 columns in the ragged ones)
    'first_none_u8_c39_last': ('conv', 'enc', NONE40, (3, 37, 70), 'forward_u8', 'u0.out', 39, LAST, {}),
    'first_gdn_f32_c0_first': ('conv', 'enc', GDN32, (3, 37, 70), 'forward', 'u0.out', 0, FIRST, {}),
    'first_gdn_u8_c39_last': ('conv', 'enc', GDN40, (3, 37, 70), 'forward_u8', 'u0.out', 39, LAST, {}),
    'first_none_f32_c31_mid': ('conv', 'enc', NONE40, (3, 37, 70), 'forward', 'u0.out', 31, (1, 16, 32), {}),
    # conv_s2_f16_kernel, S = 2, unit 1: 66 x 90 tiles -> 33 x 45 -> 17 x 23
    's2_gdn_ct1_c0_first': ('conv', 'enc', GDN32, (3, 66, 90), 'forward_u8', 'u1.out', 0, FIRST, {}),
    's2_gdn_ct2_c39_last': ('conv', 'enc', GDN40, (3, 66, 90), 'forward_u8', 'u1.out', 39, LAST, {}),
    's2_lrelu_c32_mid': ('conv', 'enc', LRELU40, (3, 66, 90), 'forward', 'u1.out', 32, (1, 16, 16), {}),
    # S = 1: reflect pre-convolution of a LeakyReLU unit (33 x 45), zero-padded one of a synthesis unit (10 x 18), residual
    's1_reflect_lrelu_c39_last': ('conv', 'enc', LRELU40, (3, 66, 90), 'forward_u8', 'u1.s0', 39, LAST, {}),
    's1_reflect_lrelu_c0_first': ('conv', 'enc', LRELU40, (3, 66, 90), 'forward', 'u1.s0', 0, FIRST, {}),
    's1_zeropad_lrelu_c39_last': ('conv', 'dec', LRELU40, (3, 5, 9), 'forward', 'u1.s0', 39, LAST, {}),
    's1_residual_sum_c39_last': ('res', 'enc', RES40, (3, 66, 90), 'forward_u8', 'u1.s0', 39, LAST, {}),
    's1_residual_sum_c8_mid': ('res', 'enc', RES40, (3, 66, 90), 'forward', 'u1.s0', 8, (1, 16, 32), {}),
    # deconv_s2_f16_kernel, unit 1: latents 5 x 9 -> 10 x 18 -> 20 x 36; one case per output parity (py, px)
    'deconv_igdn_c39_p11_last': ('conv', 'dec', GDN40, (3, 5, 9), 'forward', 'u1.out', 39, LAST, {}),
    'deconv_none_c0_p01': ('conv', 'dec', NONE40, (3, 5, 9), 'forward', 'u1.out', 0, (1, -2, -1), {}),
    'deconv_pmap_igdn_c39_p10_symbols': ('conv', 'dec', GDN40, (3, 5, 9), 'forward_symbols_u8', 'u1.out', 39, (-1, -1, -2), {}),
    'deconv_pmap_none_c0_p00_first': ('conv', 'dec', NONE40, (3, 5, 9), 'forward_u8', 'u1.out', 0, FIRST, {}),
    # gdn_f16_kernel at 192 channels: the convolution's pre-GDN store (the post-GDN value stays in range), and a post-IGDN one
    'gdn192_pre_c191_last': ('conv', 'enc', GDN192, (3, 66, 90), 'forward_u8', 'u1.pre', 191, LAST, {}),
    'igdn192_pre_c191_last': ('conv', 'dec', GDN192, (3, 5, 9), 'forward', 'u1.pre', 191, LAST, {'beta': 1e-4}),
    'igdn192_post_c0_first': ('conv', 'dec', GDN192, (3, 5, 9), 'forward', 'u1.out', 0, FIRST, {'beta': 4.0}),
    # nchw_to_c8s_kernel<false>: float tiles of 8 channels (no fused first layer)
    'tiles_f32_c7_last': ('spike', 'enc', C8, (3, 37, 70), 'forward', 'input', 7, LAST, {}),
    'tiles_f32_c0_first': ('spike', 'enc', C8, (3, 37, 70), 'forward', 'input', 0, FIRST, {}),
    'tiles_f32_c3_mid': ('spike', 'enc', C8, (3, 37, 70), 'forward', 'input', 3, (1, 16, 32), {}),
    # nchw_to_c8s_kernel<true>: latents, and the fused dequantiser (symbol + median)
    'latents_c47_last': ('spike', 'dec', LAT2, (3, 9, 23), 'forward', 'input', 47, LAST, {}),
    'latents_c0_first_u8': ('spike', 'dec', NONE40, (3, 5, 9), 'forward_u8', 'input', 0, FIRST, {}),
    'symbols_c40_mid': ('spike', 'dec', LAT2, (3, 9, 23), 'forward_symbols_u8', 'input', 40, (1, 4, 17), {}),
    # c8_to_c8s_kernel<false> / <true>: the stages of residual units above 128 channels run on the fp32 kernels
    'fp32_stages_enc_c159_last': ('res', 'enc', RES160_ENC, (3, 66, 90), 'forward_u8', 'u1.stages', 159, LAST, {}),
    'fp32_stages_dec_c159_last': ('res', 'dec', RES160_DEC, (3, 9, 17), 'forward', 'u1.stages', 159, LAST, {}),
    'fp32_stages_dec_c0_first': ('res', 'dec', RES160_DEC, (3, 9, 17), 'forward', 'u1.stages', 0, FIRST, {}),
    # scaled decode: L = 4, scale 2: units 0 and 1 run, then colour layer 1
    'scaled_decode_c31_last': ('conv', 'dec', MULTI32, (3, 5, 9), 'forward_scale', 'u1.out', 31, LAST, {}),
}


class Case:
    """One built case: the track with its edits, the call's input, the float64 result and every split-stored tensor."""

    def __init__(self, name, frac):
        self.name, self.frac = name, frac
        self.kind, self.side, kw, self.shape, self.entry, self.tensor, self.c, pos, self.extra = CASES[name]
        self.synthesis = self.side == 'dec'
        self.track, self.cfg = _track(self.side, len(name), kw)
        self.nrun = 2 if self.entry == 'forward_scale' else None
        self.med = torch.linspace(-0.4, 0.4, self.cfg['channels_bn']) if self.entry == 'forward_symbols_u8' else None
        units = self.track._units()
        t = int(self.tensor[1]) if self.tensor != 'input' else -1
        self.t = t
        # resolution of the target tensor, and its position
        n, a, b = self.shape
        up = (lambda v, k: v * 2 ** k) if self.synthesis else (lambda v, k: -(-v // 2 ** k))
        lvl = 0 if self.tensor == 'input' else (t if '.s' in self.tensor else t + 1)
        H, W = up(a, lvl), up(b, lvl)
        self.pos = tuple(p % m for p, m in zip(pos, (n, H, W)))
        self.x = self._input(lvl)
        with torch.no_grad():
            self._edit(units)
        if self.kind == 'spike':
            self._spike(frac * F16_MAX)
        else:
            self._calibrate(units, frac * F16_MAX)
        for u in units:  # (a weight beyond the f16 range would take the whole model to the fp32 kernels)
            for p in u.parameters():
                assert float(p.detach().abs().max()) < F16_MAX
        self.stored = []
        self.ref = _replay(self.track, self._x64(), self.synthesis, self.nrun,
                           hook=lambda nm, v: (self.stored.append((nm, v)), v)[1])

    # -- input: dark tiles with one bright patch / small latents with one hot pixel, below the target pixel
    def _input(self, lvl):
        n, a, b = self.shape
        s, y, x = self.pos
        rng = np.random.default_rng(len(self.name))
        if not self.synthesis:
            tiles = rng.integers(0, 12, (n, a, b, self.cfg['channels_org']), dtype=np.uint8)
            if self.kind != 'spike':
                py, px = min(y * 2 ** lvl, a - 2), min(x * 2 ** lvl, b - 2)
                tiles[s, py:py + 2, px:px + 2] = 255
            return torch.from_numpy(tiles)
        lat = torch.from_numpy(rng.standard_normal((n, self.cfg['channels_bn'], a, b)).astype(np.float32)) * 0.3
        if self.kind != 'spike':
            lat[s, :, min(y // 2 ** lvl, a - 1), min(x // 2 ** lvl, b - 1)] *= 10.0
        return torch.round(lat * 8) if self.med is not None else lat  # (symbols: integers)

    def _x64(self):
        """the call's input as the kernels read it (uint8 / 255 in fp32; symbol + median in fp32)"""
        if not self.synthesis:
            return (self.x.permute(0, 3, 1, 2).float() / 255.0 if self.x.dtype == torch.uint8 else self.x).double()
        return (self.x + self.med.view(1, -1, 1, 1) if self.med is not None else self.x).double()

    def _consumers(self, units, i):
        """the convolutions that read u{i}.out"""
        out = []
        if i + 1 < len(units):
            nxt = units[i + 1]
            out.append(_stage_conv(nxt) if R.unit_parts(nxt)[0] else nxt.main)
        if getattr(self.track, 'multiscale_analysis', False) and i + 1 < len(units):
            out.append(self.track.color_layers[i][0])
        return out

    def _edit(self, units):
        c, t = self.c, self.t
        if self.kind == 'spike':
            if not self.synthesis and self.x.dtype == torch.uint8:
                self.x = self.x.permute(0, 3, 1, 2).float() / 255.0
            first = units[0]
            _in_channel(_stage_conv(first) if R.unit_parts(first)[0] else first.main, c).zero_()
            return
        if self.entry == 'forward' and not self.synthesis:
            self.x = self.x.permute(0, 3, 1, 2).float() / 255.0
        if self.kind == 'conv':
            if '.s' in self.tensor:
                self.driver, readers = _stage_conv(units[t]), [units[t].main]
            else:
                self.driver, readers = units[t].main, self._consumers(units, t)
                if units[t].gdn is not None and (self.tensor.endswith('.out') or self.synthesis):
                    _let_through(units[t].gdn, c, self.extra.get('beta', 1.0))
            self.probe_key = self.tensor.replace('.pre', '.out') + '.in'
        else:  # 'res': x_c from the unit before, the stage adds g x_c to it
            self.driver, self.probe_key = units[t - 1].main, f'u{t - 1}.out.in'
            if units[t - 1].gdn is not None:
                _let_through(units[t - 1].gdn, c)
            st = _stage_conv(units[t])
            _in_channel(st, c).zero_()
            _out_channel(st, c).zero_()
            st.weight.data[c, c, st.kernel_size // 2, st.kernel_size // 2] = 5.0 / 6.0
            if st.bias is not None:
                st.bias.data[c] = 0.0
            if _stage_gdn(units[t]) is not None:
                _let_through(_stage_gdn(units[t]), c)
            readers = [units[t].main]
        for conv in readers:
            _in_channel(conv, c).zero_()
        if self.driver.bias is not None:
            self.driver.bias.data[c] = 0.0

    def _spike(self, value):
        s, y, x = self.pos
        if self.med is not None:  # symbol + median == value exactly (both are exact in fp32)
            self.med[self.c] = 4.0 + (value - round(value))
            self.x[s, self.c, y, x] = round(value) - 4.0
            assert float(self.x[s, self.c, y, x]).is_integer()
        else:
            self.x[s, self.c, y, x] = value

    def _calibrate(self, units, want):
        probe = {}
        _out_channel(self.driver, self.c).zero_()
        _replay(self.track, self._x64(), self.synthesis, self.nrun, probe=probe)
        xin = probe[self.probe_key]
        ks = self.track._dims[4]
        stride1 = '.s' in self.probe_key
        op = ((R.op_deconv_s1 if stride1 else R.op_deconv_s2) if self.synthesis else
              (R.op_conv_s1 if stride1 else R.op_conv_s2))(ks)
        w = torch.zeros(self.driver.weight.shape, dtype=torch.float64, requires_grad=True)
        s, y, x = self.pos
        op(xin, w)[s, self.c, y, x].backward()
        g = w.grad[:, self.c] if self.driver.transposed else w.grad[self.c]
        self.pattern = g / float((g * g).sum())  # response 1 at the target
        scale = want
        for _ in range(12):
            with torch.no_grad():
                _out_channel(self.driver, self.c).copy_((self.pattern * scale).float())
            got = self.value()
            if abs(got / want - 1.0) < 1e-4:
                return
            scale *= want / got
        raise AssertionError(f'{self.name}: no scale gives {want} at the target (last value {got})')

    def value(self):
        """the target element of the float64 replay"""
        seen = {}
        _replay(self.track, self._x64(), self.synthesis, self.nrun, hook=lambda nm, v: seen.setdefault(nm, v))
        s, y, x = self.pos
        return float(seen[self.tensor][s, self.c, y, x])

    def symbols(self):
        return self.x.to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(name, frac):
    return Case(name, frac)


NAMES = list(CASES)


# ----------------------------------------------------------------------------------------------------- the table (CPU)
def _largest(case):
    """(|value|, tensor name, index) of the largest stored element and the largest of all the others"""
    best, second = (0.0, None, None), 0.0
    for nm, v in case.stored:
        a = v.abs()
        top = torch.topk(a.flatten(), 2).values
        idx = tuple(int(i) for i in np.unravel_index(int(a.argmax()), a.shape))
        if float(top[0]) > best[0]:
            second = max(second, best[0], float(top[1]))
            best = (float(top[0]), nm, idx)
        else:
            second = max(second, float(top[0]))
    return best, second


def test_table_covers_every_site():
    """every store site of the issue, >= 3 positions per kernel site, the four parities of the transposed convolution"""
    written = {(CASES[n][1], CASES[n][5].split('.')[-1], CASES[n][4]) for n in NAMES}
    for need in [('enc', 'out', 'forward_u8'), ('enc', 'out', 'forward'), ('enc', 's0', 'forward'), ('dec', 's0', 'forward'),
                 ('dec', 'out', 'forward'), ('dec', 'out', 'forward_u8'), ('dec', 'out', 'forward_symbols_u8'),
                 ('enc', 'pre', 'forward_u8'), ('dec', 'pre', 'forward'), ('enc', 'input', 'forward'),
                 ('dec', 'input', 'forward'), ('dec', 'input', 'forward_symbols_u8'), ('enc', 'stages', 'forward_u8'),
                 ('dec', 'stages', 'forward'), ('dec', 'out', 'forward_scale')]:
        assert need in written, need
    parities = {(_case(n, OVER).pos[1] & 1, _case(n, OVER).pos[2] & 1) for n in NAMES if n.startswith('deconv_')}
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize('name', NAMES)
def test_premise_one_unstorable_value_where_the_case_says(name):
    case = _case(name, OVER)
    (top, nm, idx), second = _largest(case)
    assert top > F16_MAX and abs(top / (OVER * F16_MAX) - 1) < 1e-3, top
    assert (nm, idx) == (case.tensor, (case.pos[0], case.c) + case.pos[1:]), (nm, idx)
    assert second < UNDER * F16_MAX, second
    assert sum(int((v.abs() > F16_MAX).sum()) for _, v in case.stored) == 1
    assert bool(torch.isfinite(case.ref).all())
    if case.kind == 'res':  # both addends of the residual sum are storable
        x_c = dict(case.stored)[f'u{case.t - 1}.out'][(case.pos[0], case.c) + case.pos[1:]]
        assert 0.5 * F16_MAX < float(x_c) < 0.7 * F16_MAX and top - float(x_c) < 0.6 * F16_MAX
    if not (case.cfg['use_residual'] or case.cfg.get('multiscale_analysis')):
        # plain units: the replay is oracle/cae_oracle.py's track on the same parameters
        from oracle import cae_oracle as O
        part = 'decoder' if case.synthesis else 'encoder'
        layers = oracle_layers({part: case.track.state_dict(), 'act_layer_type': case.cfg['act_layer_type']}, part)
        fwd = O.synthesis_forward if case.synthesis else O.analysis_forward
        _close(fwd(case._x64().float(), layers)[0].double(), case.ref, 'float64 replay against the fp32 oracle')


@pytest.mark.parametrize('name', NAMES)
def test_sensitivity_a_missed_value_cannot_pass(name):
    """the target through the split format (hi = f16(v), lo = f16(v - hi)), the track continued from hi + lo"""
    case = _case(name, OVER)

    def through_split(nm, v):
        if nm != case.tensor:
            return v
        hi, lo = R.split(v)
        return hi + lo
    with np.errstate(all='ignore'):
        got = _replay(case.track, case._x64(), case.synthesis, case.nrun, hook=through_split)
    scale = max(1.0, float(case.ref.abs().max()))
    assert not bool(torch.isfinite(got).all()) or float((got - case.ref).abs().max()) / scale > RTOL


@pytest.mark.parametrize('name', NAMES)
def test_twin_stays_in_range(name):
    case = _case(name, UNDER)
    (top, nm, idx), _ = _largest(case)
    assert abs(top / (UNDER * F16_MAX) - 1) < 1e-3 and nm == case.tensor, (top, nm)
    assert all(float(v.abs().max()) <= F16_MAX for _, v in case.stored)


# ----------------------------------------------------------------------------------------------------- GPU
def _eb(med):
    from cnn_autoencoder_amd import entropy
    eb = entropy.EntropyBottleneck(med.numel()).cuda()
    with torch.no_grad():
        eb.quantiles[:, 0, 1] = med.to(eb.quantiles.device)
    eb.update(force=True)
    return eb


def _call(track, entry, x, eb=None):
    with torch.no_grad():
        if entry == 'forward_symbols_u8':
            out = track.forward_symbols_u8(x.to(torch.int32).cuda(), eb)
        elif entry == 'forward_scale':
            out = track.forward_scale(x.cuda(), 2)
        elif entry == 'forward' and isinstance(track, _synthesizer_cls()):
            out = track(x.cuda())[0][0]
        else:
            out = getattr(track, entry)(x.cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _synthesizer_cls():
    import cnn_autoencoder_amd as cae
    return cae.Synthesizer


def _close_to_oracle(got, ref, what):
    """_close; a uint8 result (x255, clip, truncate: monotone) must lie between the images of ref -+ the same tolerance"""
    if got.dtype != torch.uint8:
        return _close(got.double(), ref, what)
    tol = RTOL * max(1.0, float(ref.abs().max()))
    img = lambda v: torch.floor((255.0 * v).clamp(0, 255)).permute(0, 2, 3, 1)  # noqa: E731
    g = got.double()
    bad = (g < img(ref - tol)) | (g > img(ref + tol))
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} uint8 values outside trunc(clip(255 (ref -+ {tol:.1e})))'


def _run_both(case):
    """-> (f16x3 result, fallbacks it took, the same module's fp32 result)"""
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    track = case.track
    eb = _eb(case.med) if case.med is not None else None
    track.precision = 'f16x3'
    assert track.precision_code() == 1
    before = track.fp32_fallbacks
    got = _call(track, case.entry, case.x, eb)
    took = track.fp32_fallbacks - before
    prec = ctypes.c_int(-1)
    from cnn_autoencoder_amd import _lib
    _lib.check(_lib.lib().cae_model_effective_precision(track._sync().ptr, ctypes.byref(prec)))
    assert prec.value == 1  # the first run was on the f16x3 kernels
    track.precision = 'fp32'
    want = _call(track, case.entry, case.x, eb)
    assert track.fp32_fallbacks == before + took
    track.precision = 'f16x3'
    return got, took, want


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_one_unstorable_value_falls_back(built_lib, name):
    case = _case(name, OVER)
    got, took, fp32 = _run_both(case)
    print(f'{name}: fallbacks {took}, equal to fp32 {torch.equal(got, fp32)}')
    assert took == 1
    assert torch.equal(got, fp32)
    _close_to_oracle(got, case.ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_twin_runs_on_f16x3(built_lib, name):
    """0.9 x 65504 at the same place: invalid lanes, padding channels and ragged tiles raise nothing"""
    case = _case(name, UNDER)
    got, took, _ = _run_both(case)
    if got.dtype != torch.uint8:
        scale = max(1.0, float(case.ref.abs().max()))
        print(f'{name}: fallbacks {took}, error {float((got.double() - case.ref).abs().max()) / scale:.3e} of {scale:.3e}')
    assert took == 0
    _close_to_oracle(got, case.ref, name + ' (twin)')


# -- threshold, at the conversion sites: the stored value is set exactly
def _spike_case(name, value):
    case = Case(name, UNDER)
    case._spike(value)
    return case


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiles_f32_c7_last', 'latents_c47_last', 'symbols_c40_mid'])
def test_threshold_is_65504(built_lib, name):
    """65504 is stored; the next float32 above it (65504 + 2^-8), 65508 and -65508 are not"""
    above = float(np.nextafter(np.float32(65504.0), np.float32(np.inf)))
    assert above == 65504.0 + 2.0 ** -8
    for value, expect in ((65504.0, 0), (above, 1), (65508.0, 1), (-65508.0, 1)):
        case = _spike_case(name, value)
        assert float(case._x64()[(case.pos[0], case.c) + case.pos[1:]]) == value
        got, took, fp32 = _run_both(case)
        assert took == expect, (value, took)
        if expect:
            assert torch.equal(got, fp32)
        ref = _replay(case.track, case._x64(), case.synthesis)
        _close_to_oracle(got, ref, f'{name} at {value}')


# -- NaN and +-inf
def _same_with_nans(a, b):
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.gpu
@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', 'neg_inf'])
@pytest.mark.parametrize('name', ['tiles_f32_c7_last', 'first_gdn_f32_c0_first', 'first_none_f32_c31_mid',
                                  'latents_c47_last', 'latents_c0_first_u8'])
def test_non_finite_input_falls_back(built_lib, name, bad):
    """one NaN / inf in a float input (layout conversion, and the fused first layer that reads the tile itself) or in the
    latents: one fallback, and the fp32 module's result (NaN where it has NaN; forward_u8: the NaN-safe uint8 clip)"""
    case = Case(name, UNDER)
    s, y, x = case.pos
    case.x[s, case.c % case.x.shape[1], y, x] = bad
    got, took, fp32 = _run_both(case)
    assert took == 1
    if got.dtype == torch.uint8:
        assert torch.equal(got, fp32)
    else:
        _same_with_nans(got, fp32)


# -- ticket protocol, through the C ABI
@pytest.mark.gpu
def test_ticket_protocol(built_lib):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()

    def check(handle, ticket):
        over = ctypes.c_int(-1)
        return L.cae_range_check(handle.ptr, ctypes.c_int64(ticket), ctypes.byref(over)), over.value

    def analysis(track, x):
        hd = track._sync()
        n, _, h, w = x.shape
        y = torch.empty((n, track._dims[2]) + track.latent_size(h, w), dtype=torch.float32, device='cuda')
        _lib.check(L.cae_analysis(hd.ptr, x.data_ptr(), _lib.FMT_F32_NCHW, n, h, w, y.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return hd, int(L.cae_last_range_ticket())

    over_case, other = Case('tiles_f32_c7_last', OVER), Case('tiles_f32_c0_first', UNDER)
    x_over = over_case.x.cuda()
    small = torch.rand(1, 8, 8, 8).cuda()
    # an fp32-precision call: ticket 0, and ticket 0 reports clean
    over_case.track.precision = 'fp32'
    hd, t0 = analysis(over_case.track, x_over)
    assert t0 == 0 and check(hd, 0) == (0, 0)
    over_case.track.precision = 'f16x3'
    hd, t_over = analysis(over_case.track, x_over)
    assert t_over > 0 and check(hd, t_over) == (0, 1)
    # the word of one handle does not show on another
    hd2, t2 = analysis(other.track, other.x.cuda())
    assert t2 > 0 and check(hd2, t2) == (0, 0) and check(hd, t_over) == (0, 1)
    # 1024 slots: after 1023 further calls the ticket is still tracked, the next call reuses its slot and reports clean
    for k in range(1024):
        if k == 1023:
            assert check(hd, t_over) == (0, 1)
        _, t = analysis(over_case.track, small)
    assert t == t_over + 1024 and check(hd, t) == (0, 0)
    rc, _ = check(hd, t_over)
    assert rc == -1  # CAE_ERR_ARG
    assert b'too old' in L.cae_last_error()
