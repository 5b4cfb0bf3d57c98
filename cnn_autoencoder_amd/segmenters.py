"""Compressed-domain segmentation: the reference's ``JNet`` head (``models/tasks/_segmenters.py:307-328``) on the
quantised latents ``y_q`` and the decoder's per-level features ``fx_brg``, as ``forward_func`` hands them over
(``_taskutils.py:95-108``).  Eval-mode inference only; the hot path is ``cae_seg_forward`` (csrc/cae_seg.hip,
csrc/cae_kernels_seg.hpp).  This is analysis beside the codec, not part of it.

The module classes carry the reference's attribute names, so the ``state_dict`` keys and shapes are the reference's
and its checkpoints load with ``strict=True``.  The parameter holders are ordinary torch layers; they are never called
on the hot path.  ``force_torch=True`` runs the same head as torch ops on the device (the measurement's comparison and
a second opinion in the tests).  Not built, and raising ``NotImplementedError``: ``UNet`` with its own analysis track
(image domain, ``MaxPool``).  Training lives beside this module: ``seg_train.JNetTrain`` is this ``JNet`` with a backward
pass (same state dict), with the loader, forward function, losses and step of the reference's head training; this
``JNet`` itself refuses train mode and calls while autograd is recording.

The head's structure is stated once, in the library (``cae_seg_plan``); ``JNet.stage_plan()`` mirrors it with the tensors.

``predict`` / ``class_metrics`` turn logits into what the reference's harness hands out (class map, scores, counts and
metrics; ``cae_seg_predict``, csrc/cae_seg_predict.hip); ``slide.SlideCoder.segment_batches`` and ``zarrio.segment_image``
run whole slides through codec, head and prediction.  ``roc_histogram`` / ``roc_from_histogram`` give the threshold-free
results of a one-class head, ROC curve and AUC, from exact logit histograms (``cae_seg_roc_hist``, csrc/cae_seg_hist.hip).
``score_histogram`` / ``ap_from_histogram`` give the average precision of a head of several classes, with bounds on that of
the unbinned scores, from exact histograms of the softmax scores (``cae_seg_score_hist``, csrc/cae_seg_hist.hip).
``components`` / ``object_cover`` / ``object_counts`` / ``object_roc_histogram`` give the object-level half of the harness:
connected objects of the target, their boxes, and counts and histogram over the pixels of all boxes (csrc/cae_seg_objects.hip).

Unlike the reference (whose in-place ReLU overwrites the caller's bridges when ``batch_norm=False``) the head never
writes its inputs.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

F16_MAX = 65504.0
EPS = 1e-5


def _norm(channels: int, batch_norm: bool) -> nn.Module:
    return nn.GroupNorm(num_groups=channels, num_channels=channels) if batch_norm else nn.Identity()


def _conv3(cin: int, cout: int) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=False)


def _up2(cin: int, cout: int) -> nn.ConvTranspose2d:
    return nn.ConvTranspose2d(cin, cout, kernel_size=2, stride=2, padding=0, output_padding=0, bias=True)


class _Holder(nn.Module):
    """Parameter holder of one unit: the head's forward runs all units in one library call."""

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__} is not callable on its own: call the JNet that owns it')


class ProjectionUnit(_Holder):
    """GN, ReLU, 3x3 conv, GN, ReLU on a bridge."""

    def __init__(self, channels_in, channels_out, kernel_size=3, batch_norm=True):
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError('the segmentation head is built for kernel_size=3')
        self._bn1 = _norm(channels_in, batch_norm)
        self._c2 = _conv3(channels_in, channels_out)
        self._bn2 = _norm(channels_out, batch_norm)
        self._relu = nn.ReLU(inplace=False)


class UpsamplingUnit(_Holder):
    """3x3 conv, GN, ReLU, 3x3 conv, GN, ReLU, then the 2x2 stride-2 transposed conv (identity at the last level)."""

    def __init__(self, channels_in, channels_unit, channels_out, kernel_size=3, batch_norm=True, upsample=True):
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError('the segmentation head is built for kernel_size=3')
        self._c1 = _conv3(channels_in, channels_unit)
        self._bn1 = _norm(channels_unit, batch_norm)
        self._c2 = _conv3(channels_unit, channels_unit)
        self._bn2 = _norm(channels_unit, batch_norm)
        self._relu = nn.ReLU(inplace=False)
        self._up_sample = _up2(channels_unit, channels_out) if upsample else nn.Identity()


class BottleneckUnit(_Holder):
    """As JNet patches it: 1x1 conv on the raw latents (no pooling), GN, ReLU, 3x3 conv, GN, ReLU, transposed conv."""

    def __init__(self, channels_latent, channels_in, channels_out, batch_norm=True):
        super().__init__()
        self._dwn_sample = nn.Identity()
        self._c1 = nn.Conv2d(channels_latent, channels_out, kernel_size=1, stride=1, padding=0, bias=False)
        self._bn1 = _norm(channels_out, batch_norm)
        self._c2 = _conv3(channels_out, channels_out)
        self._bn2 = _norm(channels_out, batch_norm)
        self._relu = nn.ReLU(inplace=False)
        self._up_sample = _up2(channels_out, channels_in)


class UNet(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError('UNet with its own analysis track (image domain, MaxPool) is not built: only JNet, the '
                                  'synthesis track on latents and decoder bridges, is')


class _SegConfig(ctypes.Structure):
    _fields_ = [('channels_bn', ctypes.c_int), ('seg_channels_bn', ctypes.c_int), ('levels', ctypes.c_int),
                ('num_classes', ctypes.c_int), ('concat_bridges', ctypes.c_int), ('batch_norm', ctypes.c_int),
                ('bridge_channels', ctypes.c_int * 8), ('level_channels', ctypes.c_int * 8),
                ('up_channels', ctypes.c_int * 8)]


class _SegTaps(ctypes.Structure):
    _fields_ = [('raw', ctypes.POINTER(ctypes.c_void_p)), ('ab', ctypes.POINTER(ctypes.c_void_p)),
                ('bridge_ab', ctypes.POINTER(ctypes.c_void_p))]


class _SegHandle:
    """Owns one cae_seg_t."""

    def __init__(self, cfg: _SegConfig, weights: Sequence[np.ndarray]):
        self._h = ctypes.c_void_p()
        ptrs = (ctypes.c_void_p * len(weights))(*[w.ctypes.data for w in weights])
        _lib.check(_lib.lib().cae_seg_create(ctypes.byref(cfg), ptrs, len(weights), ctypes.byref(self._h)))

    @property
    def ptr(self):
        return self._h

    def close(self):
        if self._h:
            _lib.lib().cae_seg_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JNet(nn.Module):
    def __init__(self, seg_channels_net=64, channels_bn=320, seg_channels_bn=1024, seg_channels_expansion=2,
                 compression_level=4, concat_bridges=False, channels_org=3, channels_net=64, channels_expansion=1,
                 num_classes=1, batch_norm=True, force_torch=False, **kwargs):
        # (unknown kwargs -- save_bridges, channels_prg, the codec's own keys -- are swallowed as in the reference)
        super().__init__()
        L = int(compression_level)
        if not 1 <= L <= 8:
            raise ValueError(f'compression_level {compression_level} outside 1..8')
        self._concat_bridges = bool(concat_bridges)
        self._batch_norm = bool(batch_norm)
        self.force_torch = bool(force_torch)
        self._channels_bn = int(channels_bn)
        self._num_classes = int(num_classes)
        self._bridge_channels = [int(channels_net * channels_expansion ** c) for c in range(L - 1)] + [int(channels_org)]
        self._level_channels = [int(seg_channels_net * seg_channels_expansion ** c) for c in reversed(range(L))]
        self._up_channels = [int(seg_channels_net * seg_channels_expansion ** (c - 1)) for c in reversed(range(L))]
        self._seg_channels_bn = int(seg_channels_bn)
        self.analysis_track: List = []

        proj, track = [], []
        for i in range(L):
            ch = self._level_channels[i]
            proj.append(ProjectionUnit(self._bridge_channels[i], ch, batch_norm=batch_norm) if concat_bridges
                        else nn.Identity())
            track.append(UpsamplingUnit(ch * 2 ** int(bool(concat_bridges)), ch, self._up_channels[i],
                                        batch_norm=batch_norm, upsample=i + 1 < L))
        self.bridges_projection = nn.ModuleList(proj)
        self.synthesis_track = nn.ModuleList(track)
        self.bottleneck = BottleneckUnit(self._channels_bn, self._level_channels[0], self._seg_channels_bn,
                                         batch_norm=batch_norm)
        self.fc = nn.Conv2d(int(seg_channels_net), self._num_classes, kernel_size=1, stride=1, padding=0, bias=True)
        self._handle: Optional[_SegHandle] = None
        self._uploaded = None

    # ---- the head as a list of stages, in the library's launch order -----------------------------------------
    def stage_plan(self) -> List[Dict]:
        """One entry per convolution: name, ks, up (2x2 stride-2 transposed), weight, bias, norm (the GroupNorm behind
        it, or None), and its sources in contraction order: ('latent',), ('bridge', i) (normalised by the projection's
        _bn1, then ReLU), ('raw', s, True) (stage s's output through its (a, b) and ReLU) or ('raw', s, False)
        (untransformed)."""
        bn = self._batch_norm
        plan: List[Dict] = []

        def add(name, conv, srcs, norm=None, up=False):
            plan.append(dict(name=name, ks=1 if up else conv.kernel_size[0], up=up, weight=conv.weight, bias=conv.bias,
                             norm=norm if bn else None, has_ab=norm is not None, srcs=srcs))
            return len(plan) - 1

        b = self.bottleneck
        s = add('bottleneck._c1', b._c1, [('latent',)], b._bn1)
        s = add('bottleneck._c2', b._c2, [('raw', s, True)], b._bn2)
        up = add('bottleneck._up_sample', b._up_sample, [('raw', s, True)], up=True)
        for i, (p, u) in enumerate(zip(self.bridges_projection, self.synthesis_track)):
            srcs = [('raw', up, False)]
            if self._concat_bridges:
                s = add(f'bridges_projection.{i}._c2', p._c2, [('bridge', i)], p._bn2)
                srcs = [('raw', s, True)] + srcs
            s = add(f'synthesis_track.{i}._c1', u._c1, srcs, u._bn1)
            s = add(f'synthesis_track.{i}._c2', u._c2, [('raw', s, True)], u._bn2)
            if i + 1 < len(self.synthesis_track):
                up = add(f'synthesis_track.{i}._up_sample', u._up_sample, [('raw', s, True)], up=True)
        add('fc', self.fc, [('raw', s, True)])
        return plan

    def _weight_list(self) -> List[torch.Tensor]:
        out: List[torch.Tensor] = []
        for i, st in enumerate(self.stage_plan()):
            if st['srcs'][0][0] == 'bridge' and self._batch_norm:
                bn1 = self.bridges_projection[st['srcs'][0][1]]._bn1
                out += [bn1.weight, bn1.bias]
            out.append(st['weight'])
            if st['bias'] is not None:
                out.append(st['bias'])
            if st['norm'] is not None:
                out += [st['norm'].weight, st['norm'].bias]
        return out

    def _config(self) -> _SegConfig:
        cfg = _SegConfig()
        cfg.channels_bn, cfg.seg_channels_bn = self._channels_bn, self._seg_channels_bn
        cfg.levels, cfg.num_classes = len(self.synthesis_track), self._num_classes
        cfg.concat_bridges, cfg.batch_norm = int(self._concat_bridges), int(self._batch_norm)
        for i in range(cfg.levels):
            cfg.bridge_channels[i] = self._bridge_channels[i]
            cfg.level_channels[i] = self._level_channels[i]
            cfg.up_channels[i] = self._up_channels[i]
        return cfg

    def _sync(self) -> _SegHandle:
        ws = self._weight_list()
        version = tuple((w.data_ptr(), w._version) for w in ws)
        if self._handle is None or version != self._uploaded:
            host = [np.ascontiguousarray(w.detach().cpu().float().numpy()) for w in ws]
            handle = _SegHandle(self._config(), host)  # ValueError: a weight, gamma or beta outside the f16 range
            if self._handle is not None:
                self._handle.close()
            self._handle, self._uploaded = handle, version
        return self._handle

    # ---- call surface --------------------------------------------------------------------------------------------
    def _check(self, x, fx_brg):
        if self.training:
            raise NotImplementedError('training the segmentation head is not built: call .eval() (GroupNorm keeps no '
                                      'running statistics, eval mode normalises by the data as train mode does)')
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError('the segmentation head has no backward pass: call it under torch.no_grad()')
        if x.dim() != 4 or x.size(1) != self._channels_bn:
            raise ValueError(f'expected latents (B,{self._channels_bn},h,w), got {tuple(x.shape)}')
        if not self._concat_bridges:
            return None
        L = len(self.synthesis_track)
        if fx_brg is None or len(fx_brg) != L:
            raise ValueError(f'concat_bridges=True needs {L} bridges (Synthesizer.forward returns them), got '
                             f'{None if fx_brg is None else len(fx_brg)}')
        n, _, lh, lw = x.shape
        for i, b in enumerate(fx_brg):
            want = (n, self._bridge_channels[i], lh * 2 ** (i + 1), lw * 2 ** (i + 1))
            if b.dim() != 4 or tuple(b.shape) != want:
                raise ValueError(f'bridge {i}: expected {want}, got {tuple(b.shape)}')
        return list(fx_brg)

    def forward(self, x: torch.Tensor, fx_brg=None, taps: bool = False):
        """y_q (B,channels_bn,h,w), fx_brg: the decoder's bridges (coarsest first, the reconstruction last) ->
        (logits (B,num_classes,h 2^L,w 2^L), None).  taps=True (tests): (logits, dict of every stage's raw output and
        (a, b) pairs)."""
        x, brg = self._stage(x, self._check(x, fx_brg))
        if self.force_torch:
            return self._forward_torch(x, brg), None
        logits, tapped, ticket = self._launch(x, brg, taps)
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.lib().cae_seg_range_check(self._handle.ptr, ticket))  # FloatingPointError: never wrong logits
        return logits, tapped

    def _stage(self, x, fx_brg):
        """the checked inputs as constants on the device -> (latents, list of bridges), contiguous fp32"""
        dev = _lib.require_gpu()
        put = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        return put(x), [put(b) for b in fx_brg or []]

    def _taps(self, x, brg) -> Dict:
        """the taps of stage_plan(): raw outputs (cae_seg_forward writes each whole), (a, b) pairs, the bridges' pairs"""
        n, _, lh, lw = x.shape
        pairs = lambda c: torch.zeros((n, (c + 7) // 8 * 8, 2), dtype=torch.float32, device=x.device)
        plan, raw, ab, size = self.stage_plan(), [], [], (lh, lw)
        for st in plan:
            cout = st['weight'].shape[1 if st['up'] else 0]
            if st['up']:
                size = (2 * size[0], 2 * size[1])
            raw.append(torch.empty((n, cout) + size, dtype=torch.float32, device=x.device))
            ab.append(pairs(cout) if st['has_ab'] else None)
        return dict(plan=plan, raw=raw, ab=ab, bridge_ab=[pairs(b.size(1)) for b in brg])

    def _launch(self, x, brg, taps: bool):
        """one cae_seg_forward of staged inputs, asynchronous on the current stream -> (logits, the taps or None, the
        call's range ticket, to be checked once the stream work has completed)"""
        hd = self._sync()
        n, _, lh, lw = x.shape
        L = len(self.synthesis_track)
        logits = torch.empty((n, self._num_classes, lh * 2 ** L, lw * 2 ** L), dtype=torch.float32, device=x.device)
        brg_ptr = (ctypes.c_void_p * L)(*[b.data_ptr() for b in brg]) if brg else None
        tap_arg = tapped = None
        if taps:
            tapped = self._taps(x, brg)
            arr = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
            keep = [arr(tapped[k]) for k in ('raw', 'ab', 'bridge_ab')]
            tap_arg = ctypes.byref(_SegTaps(*[ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) for a in keep]))
        lib = _lib.lib()
        _lib.check(lib.cae_seg_forward(hd.ptr, x.data_ptr(), brg_ptr, n, lh, lw, logits.data_ptr(), tap_arg,
                                       _lib.stream_ptr()))
        return logits, tapped, lib.cae_seg_last_ticket()

    def _forward_torch(self, x: torch.Tensor, brg: List[torch.Tensor]) -> torch.Tensor:
        """The same head as torch ops on the device."""
        def gn(v, norm):
            return v if isinstance(norm, nn.Identity) else F.group_norm(v, norm.num_groups, norm.weight, norm.bias, EPS)

        def unit(v, u):
            v = F.relu(gn(F.conv2d(v, u._c1.weight, padding=u._c1.padding), u._bn1))
            v = F.relu(gn(F.conv2d(v, u._c2.weight, padding=1), u._bn2))
            up = u._up_sample
            return v if isinstance(up, nn.Identity) else F.conv_transpose2d(v, up.weight, up.bias, stride=2)

        fx = unit(x, self.bottleneck)
        for i, (p, u) in enumerate(zip(self.bridges_projection, self.synthesis_track)):
            if self._concat_bridges:
                b = F.relu(gn(brg[i], p._bn1))
                b = F.relu(gn(F.conv2d(b, p._c2.weight, padding=1), p._bn2))
                fx = torch.cat((b, fx), dim=1)
            fx = unit(fx, u)
        return F.conv2d(fx, self.fc.weight, self.fc.bias)


SEG_MODELS = {'UNet': UNet, 'JNet': JNet}


def setup_modules(segment_model_type, **kwargs):
    return SEG_MODELS[segment_model_type](**kwargs)


def load_state_dict(model, checkpoint_state):
    if 'seg_model' in checkpoint_state.keys():
        model.load_state_dict(checkpoint_state['seg_model'])


def load_segmenter(checkpoint, setup, train, trainable):
    """The loader behind both ``segmenter_from_state_dict``: ``setup(**state)`` builds the module, ``trainable`` says
    whether it has a backward pass (then ``train`` also sets the parameters' requires_grad)."""
    state = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, str) else checkpoint
    if state.get('segment_model_type', None) not in SEG_MODELS:
        raise ValueError(f"segment_model_type must be one of {sorted(SEG_MODELS)}, got {state.get('segment_model_type')!r}")
    if train and not trainable:
        raise NotImplementedError('training the segmentation head is not built (train=True)')
    model = setup(**state)
    load_state_dict(model, state)
    if torch.cuda.is_available():
        model.cuda()
    model.train(bool(train))
    for p in model.parameters() if trainable else ():
        p.requires_grad_(bool(train))
    return model


def segmenter_from_state_dict(checkpoint, gpu=False, train=False):
    """checkpoint: path or dict with 'segment_model_type', the constructor's keys and 'seg_model' (the state dict).
    ``gpu`` is accepted for signature compatibility: the head always runs on the current HIP device."""
    return load_segmenter(checkpoint, setup_modules, train, trainable=False)


@torch.no_grad()
def segment_compressed(bufs: Sequence[bytes], model, seg_model) -> torch.Tensor:
    """Codec chunk byte strings of one tile size -> logits (B, classes, H, W): range decoding, the synthesis track with
    its bridges, the head.  ``model``: the module dict of ``autoencoder_from_state_dict`` (or a
    ``ConvolutionalAutoencoder``); ``seg_model``: a ``JNet`` in eval mode."""
    from .codec import _module
    model = getattr(model, '_model', model)
    dec, eb = _module(model['decoder']), _module(model['fact_ent'])
    level = len(dec.synthesis_track)
    hw = {struct.unpack('>QQ', bytes(b[:16])) for b in bufs}
    if len(hw) != 1:
        raise ValueError('segment_compressed needs chunks of one tile size')
    h, w = hw.pop()
    lh, lw = h // 2 ** level, w // 2 ** level
    dev = _lib.require_gpu()
    sym_host = eb.decode_symbols([bytes(b[16:]) for b in bufs], lh * lw)
    sym = torch.from_numpy(sym_host).to(dev).reshape(len(bufs), eb.channels, lh, lw)
    y_q = eb.dequantize_symbols(sym)
    _, fx_brg = dec(y_q)
    return _module(seg_model)(y_q, fx_brg=fx_brg)[0]


# ---- what the reference's harness makes of the logits (test_cae_classifier.py:46-55, utils/_metrics.py:79-193) -------
COUNT_KEYS = ('tp', 'tn', 'fp', 'fn', 'p', 'tp_top')  # the columns of a counts record


def threshold_logit(threshold: float, threshold_on: str = 'scores') -> float:
    """The fp32 value the one-class logits are compared with.  'scores': the logit of the score threshold,
    float32(log(thr / (1 - thr))) evaluated in double, so that ``sigmoid(x) > thr`` (compute_metrics_per_image,
    _metrics.py:172) becomes an exact fp32 compare the host can replay; 'logits': the threshold itself, compared with the
    logit as save_pred2zarr does (test_cae_classifier.py:54)."""
    thr = float(threshold)
    if threshold_on == 'logits':
        if not np.isfinite(thr):
            raise ValueError(f'threshold must be finite, got {threshold!r}')
        return float(np.float32(thr))
    if threshold_on != 'scores':
        raise ValueError(f"threshold_on must be 'scores' or 'logits', got {threshold_on!r}")
    if not 0.0 < thr < 1.0:
        raise ValueError(f"a threshold on the scores lies inside (0, 1), got {threshold!r}")
    return float(np.float32(np.log(np.float64(thr) / (1.0 - np.float64(thr)))))


def _check_top_k(top_k) -> int:
    if int(top_k) != top_k or top_k < 1:
        raise ValueError(f'top_k must be a positive integer, got {top_k!r}')
    return int(top_k)


def _logits_arg(logits):
    """fp32 logits (N,C,...) on the device, 1..256 classes, non-empty planes -> (contiguous, n, c, space, pixels)"""
    _lib.require_gpu()
    if not isinstance(logits, torch.Tensor) or logits.dim() < 2 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise ValueError('expected fp32 logits (N,C,...) on the device')
    if not 1 <= logits.size(1) <= 256:
        raise ValueError(f'{logits.size(1)} classes outside 1..256')
    n, c, space = logits.size(0), logits.size(1), tuple(logits.shape[2:])
    hw = int(np.prod(space)) if space else 1
    if n and hw < 1:
        raise ValueError(f'empty planes: {tuple(logits.shape)}')
    return logits.contiguous(), n, c, space, hw  # (a view of a larger buffer at any element offset is read in place)


def _one_class_logits_arg(logits):
    """fp32 logits (N,1,H,W) of a one-class head on the device, non-empty planes -> (contiguous, n, h, w)"""
    _lib.require_gpu()
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise ValueError('expected fp32 logits (N,1,H,W) on the device')
    if logits.size(1) != 1:
        raise ValueError(f'the ROC histogram is built for a one-class head, got {logits.size(1)} classes')
    n, _, h, w = logits.shape
    if n and (h < 1 or w < 1):
        raise ValueError(f'empty planes: {tuple(logits.shape)}')
    return logits.contiguous(), n, h, w  # (a view of a larger buffer at any element offset is read in place)


def _target_arg(target, dev, *dims) -> torch.Tensor:
    """a uint8 target of dims[0] x dims[1] ... labels -> on the device, contiguous"""
    if not isinstance(target, torch.Tensor) or target.dtype != torch.uint8 or target.numel() != int(np.prod(dims)):
        raise ValueError(f"expected a uint8 target of {' x '.join(str(d) for d in dims)} labels")
    return target.to(dev).contiguous()


def _workspace(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max((int(nbytes) + 7) // 8, 1), dtype=torch.int64, device=dev)


def _ptr(v):
    return None if v is None else v.data_ptr()


@torch.no_grad()
def predict(logits: torch.Tensor, target: Optional[torch.Tensor] = None, threshold: float = 0.5,
            threshold_on: str = 'scores', top_k: int = 5, scores: bool = False) -> Dict:
    """logits (N,C,...) fp32 on the device, read as they stand -> dict(cls, scores, counts) on the device
    (cae_seg_predict, csrc/cae_seg_predict.hip; asynchronous on the current stream).
    cls (N,...) uint8: ``logit > threshold_logit(...)`` for one class, else the index of the largest logit (the lowest
    of equal ones).  scores (N,C,...) fp32 when asked for: sigmoid / softmax.  counts (N,6) int64
    [tp, tn, fp, fn, p, tp_top] per image when a ``target`` (N,...) uint8 is given: one class -- the confusion table of
    cls against target > 0; several -- tp = #{cls == target}, fp = fn = pixels - tp, tp_top = #{target among the
    min(top_k, C) largest logits}."""
    t = threshold_logit(threshold, threshold_on)  # ValueError before anything else
    top_k = _check_top_k(top_k)
    logits, n, c, space, hw = _logits_arg(logits)
    dev = logits.device
    tgt = None if target is None else _target_arg(target, dev, n, hw)
    with torch.cuda.device(dev):
        cls = torch.empty((n,) + space, dtype=torch.uint8, device=dev)
        sc = torch.empty_like(logits) if scores else None
        counts = ws = None
        L = _lib.lib()
        if tgt is not None:
            counts = torch.empty((n, len(COUNT_KEYS)), dtype=torch.int64, device=dev)
            ws = _workspace(L.cae_seg_predict_workspace(n, c, hw), dev)
        _lib.check(L.cae_seg_predict(logits.data_ptr(), _ptr(tgt), n, c, max(hw, 1), t, top_k, cls.data_ptr(), _ptr(sc),
                                     _ptr(counts), _ptr(ws), 0 if ws is None else ws.numel() * 8, _lib.stream_ptr()))
    return dict(cls=cls, scores=sc, counts=counts)


def class_metrics(counts, multiclass: bool = False) -> Dict:
    """One counts record [tp, tn, fp, fn, p, tp_top] -- a tile's, or the sum of many tiles' -- (or an (M,6) array of
    them, which is summed) -> the reference's metrics dictionary: tp tp_top tn fp fn p n acc top_acc prec rec f1, by the
    formulas of compute_class_metrics_dask (_metrics.py:50-59; tn_top = tn).  A zero denominator gives 0.0 for prec /
    rec / f1 (sklearn's zero_division=0 of the per-image variant) and NaN for acc / top_acc.  ``n`` = tn + fp, the
    negatives of the confusion table; ``multiclass``: the reference's 0 for records of several classes (_metrics.py:105)."""
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    rec = np.asarray(counts, dtype=np.int64)
    if rec.ndim == 2 and rec.shape[1] == len(COUNT_KEYS):
        rec = rec.sum(axis=0)
    if rec.shape != (len(COUNT_KEYS),):
        raise ValueError(f'expected a counts record of {len(COUNT_KEYS)} integers, got shape {rec.shape}')
    tp, tn, fp, fn, p, tp_top = (int(v) for v in rec)
    total = tp + tn + fp + fn
    ratio = lambda a, b: a / b if b > 0 else 0.0
    return dict(tp=tp, tp_top=tp_top, tn=tn, fp=fp, fn=fn, p=p, n=0 if multiclass else tn + fp,
                acc=(tp + tn) / total if total > 0 else float('nan'),
                top_acc=(tp_top + tn) / total if total > 0 else float('nan'),
                prec=ratio(tp, tp + fp), rec=ratio(tp, tp + fn), f1=ratio(2 * tp, 2 * tp + fp + fn))


# ---- threshold-free results of a one-class head: ROC curve and AUC from logit histograms (csrc/cae_seg_hist.hip) ------
ROC_BITS = 14          # bins of the slide histograms: 2^14 per class, the most cae_seg_roc_hist takes
ROC_BITS_RANGE = (8, 14)


def _check_bits(bits, what: str, bits_range) -> int:
    if isinstance(bits, bool) or int(bits) != bits or not bits_range[0] <= int(bits) <= bits_range[1]:
        raise ValueError(f'{what} bits must be an integer in {bits_range[0]}..{bits_range[1]}, got {bits!r}')
    return int(bits)


def _check_roc_bits(bits) -> int:
    return _check_bits(bits, 'roc', ROC_BITS_RANGE)


def _histogram_arg(hist, bits_range):
    """One integer histogram (2, B), or an (M, 2, B) array of them, which is summed; B a power of two in range, no
    negative count -> (neg, pos, N, P, bits)"""
    if isinstance(hist, torch.Tensor):
        hist = hist.detach().cpu().numpy()
    hist = np.asarray(hist)
    if hist.dtype.kind not in 'iu' or hist.ndim not in (2, 3) or hist.shape[-2] != 2:
        raise ValueError(f'expected integer histograms (2, B) or (M, 2, B), got {hist.dtype} {hist.shape}')
    hist = hist.astype(np.int64)
    if hist.ndim == 3:
        hist = hist.sum(axis=0)
    B = hist.shape[1]
    bits = B.bit_length() - 1
    if B != 1 << bits or not bits_range[0] <= bits <= bits_range[1] or (hist < 0).any():
        raise ValueError(f'expected non-negative counts in 2^{bits_range[0]}..2^{bits_range[1]} bins, got {B}')
    neg, pos = hist[0], hist[1]
    return neg, pos, int(neg.sum()), int(pos.sum()), bits


def roc_bin_edges(bits: int = ROC_BITS) -> np.ndarray:
    """float32 (2^bits,): e_j, the smallest non-NaN fp32 value of bin j of cae_seg_roc_hist (include/cae_hip.h), NaN where
    a bin holds NaN bit patterns only.  ``bin(x) >= j`` exactly when ``x >= e_j``, i.e. ``x > nextafter(e_j, -inf)``."""
    bits = _check_roc_bits(bits)
    shift = 32 - bits
    low = np.arange(1 << bits, dtype=np.uint64) << np.uint64(shift)  # the lowest key of every bin
    neg = low < (1 << 31)
    # negative floats: key = ~u, keys below that of -inf (0x007fffff) are NaN patterns; the rest: key = u | 2^31
    key = np.where(neg, np.maximum(low, 0x007FFFFF), low)
    u = np.where(neg, ~key & np.uint64(0xFFFFFFFF), key & np.uint64(0x7FFFFFFF))
    valid = np.where(neg, key < low + (1 << shift), u <= 0x7F800000)
    edges = u.astype(np.uint32).view(np.float32).copy()
    edges[~valid] = np.nan
    return edges


def _roc_histogram(logits, target, cover, extent, bits, per_image) -> torch.Tensor:
    """roc_histogram, or with a ``cover`` object_roc_histogram"""
    bits = _check_roc_bits(bits)
    logits, n, h, w = _one_class_logits_arg(logits)
    dev = logits.device
    tgt = _target_arg(target, dev, n, h, w)
    cov = None if cover is None else _check_cover(cover, n, h * w, dev)
    ext = _extent_arg(extent, n, dev)
    m = n if per_image else 1
    with torch.cuda.device(dev):
        if n == 0:
            return torch.zeros((m, 2, 1 << bits) if per_image else (2, 1 << bits), dtype=torch.int64, device=dev)
        L = _lib.lib()
        hist = torch.empty((m, 2, 1 << bits), dtype=torch.int64, device=dev)
        tail = (_ptr(ext), n, h, w, bits, int(bool(per_image)), hist.data_ptr())
        if cov is None:
            ws = _workspace(L.cae_seg_roc_workspace(n, h, w, bits), dev)
            rc = L.cae_seg_roc_hist(logits.data_ptr(), tgt.data_ptr(), *tail, ws.data_ptr(), ws.numel() * 8,
                                    _lib.stream_ptr())
        else:
            ws = _workspace(L.cae_seg_object_roc_workspace(n, h, w, bits), dev)
            rc = L.cae_seg_object_roc_hist(logits.data_ptr(), tgt.data_ptr(), cov.data_ptr(), *tail, ws.data_ptr(),
                                           ws.numel() * 8, _lib.stream_ptr())
        _lib.check(rc)
    return hist if per_image else hist[0]


@torch.no_grad()
def roc_histogram(logits: torch.Tensor, target: torch.Tensor, extent=None, bits: int = ROC_BITS,
                  per_image: bool = False) -> torch.Tensor:
    """fp32 logits (N,1,H,W) of a one-class head on the device, read as they stand, and a uint8 target (N,H,W) ->
    int64 CUDA tensor (2, 2^bits) -- row 0 the negatives' (target == 0), row 1 the positives' counts per logit bin, summed
    over the batch -- or (N, 2, 2^bits) with ``per_image`` (cae_seg_roc_hist; asynchronous on the current stream).
    ``extent``: (N,2) integers (rows, cols): only the pixels y < rows, x < cols of each image are counted (values are
    clamped to the plane).  Histograms are exact and add; ``roc_from_histogram`` makes curve and AUC of them."""
    return _roc_histogram(logits, target, None, extent, bits, per_image)


def roc_from_histogram(hist) -> Dict:
    """One histogram (2, B) of roc_histogram -- a tile's, or the sum of many tiles' -- or an (M, 2, B) array of them,
    which is summed -> dict(fpr, tpr, thresholds, score_thresholds, auc, auc_slack, p, n); pure numpy on the host.
    The curve starts at (0, 0) with threshold +inf and has one point per non-empty bin from the top down, at the bin's
    edge e_j (``thresholds``, logits; ``score_thresholds``: their sigmoid in float64): fpr / tpr are the fp / (fp + tn)
    and tp / (tp + fn) of ``predict(..., threshold=nextafter(e_j, -inf), threshold_on='logits')``, and the arrays are
    sklearn's ``roc_curve(target, logits, drop_intermediate=False)`` for logits that sit on bin edges.
    ``auc``: the trapezoid area under that curve, sum_b pos_b (2 neg_below_b + neg_b) / (2 P N) in Python integers with one
    division; the AUC of the unbinned logits lies inside auc +- ``auc_slack`` = sum_b pos_b neg_b / (2 P N).  Both are NaN
    without positives (the reference's rule, _metrics.py:128-131) or without negatives; fpr / tpr are then NaN too."""
    neg, pos, N, P, bits = _histogram_arg(hist, ROC_BITS_RANGE)
    full = np.flatnonzero(neg + pos)[::-1]  # the non-empty bins from the top down
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        fpr = np.concatenate(([0.0], np.cumsum(neg[full]) / np.float64(N))) if N else np.full(full.size + 1, np.nan)
        tpr = np.concatenate(([0.0], np.cumsum(pos[full]) / np.float64(P))) if P else np.full(full.size + 1, np.nan)
        thr = np.concatenate(([np.inf], roc_bin_edges(bits)[full].astype(np.float64)))
        score_thr = np.concatenate(([np.inf], 1.0 / (1.0 + np.exp(-thr[1:]))))
    auc = slack = float('nan')
    if P and N:
        area = ties = 0
        neg_below = np.concatenate(([0], np.cumsum(neg)[:-1]))
        for b in np.flatnonzero(pos):  # Python integers: a slide's pos_b neg_b does not fit 64 bits
            pb, nb = int(pos[b]), int(neg[b])
            area += pb * (2 * int(neg_below[b]) + nb)
            ties += pb * nb
        auc, slack = area / (2 * P * N), ties / (2 * P * N)
    return dict(fpr=fpr, tpr=tpr, thresholds=thr, score_thresholds=score_thr, auc=auc, auc_slack=slack, p=P, n=N)


# ---- average precision from score histograms (csrc/cae_seg_hist.hip); a one-class head's from its ROC histogram ------
AP_BITS = 14           # bins of the slide histograms: 2^14 per row, the most cae_seg_score_hist takes
AP_BITS_RANGE = (8, 14)


def _check_ap_bits(bits) -> int:
    return _check_bits(bits, 'ap', AP_BITS_RANGE)


def score_bin_edges(bits: int = AP_BITS) -> np.ndarray:
    """float32 (2^bits,): e_j, the smallest score in [0, 1] of bin j of cae_seg_score_hist (include/cae_hip.h), NaN for
    the bins that no fp32 score reaches: those between the two halves, and near 1 those whose values of 1 - s are no
    multiple of 2^-24.  For a score s in [0, 1], ``bin(s) >= j`` exactly when ``s >= e_j``."""
    bits = _check_ap_bits(bits)
    B, sh = 1 << bits, 31 - bits
    half = 0x3F000000 >> sh  # bits_of(0.5f) >> sh: the lower half's bins are 0 .. half - 1
    edges = np.full(B, np.nan, dtype=np.float32)
    edges[:half] = (np.arange(half, dtype=np.uint32) << np.uint32(sh)).view(np.float32)
    # upper half: bin B - 1 - q holds t = 1 - s with bits_of(t) >> sh == q; s is a multiple of 2^-24 there, so t is one
    # too, and the smallest s belongs to the largest such t.  All of it exact in float64
    q = np.arange(half + 1, dtype=np.uint32)
    t_min = (q << np.uint32(sh)).view(np.float32).astype(np.float64)
    t_max = np.minimum((((q + np.uint32(1)) << np.uint32(sh)) - np.uint32(1)).view(np.float32).astype(np.float64), 0.5)
    k = np.floor(t_max * 2.0 ** 24)
    reached = k >= t_min * 2.0 ** 24
    edges[B - 1 - q[reached]] = (1.0 - k[reached] * 2.0 ** -24).astype(np.float32)
    return edges


def _scores_arg(scores):
    """fp32 scores (N,C,H,W) of a head of 2..255 classes on the device, non-empty planes -> (contiguous, n, c, h, w)"""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 4 or scores.dtype != torch.float32:
        raise ValueError('expected fp32 scores (N,C,H,W) on the device')
    n, c, h, w = scores.shape
    if not 2 <= c <= 255:
        raise ValueError(f'the score histogram is built for heads of 2..255 classes, got {c}: a one-class head has '
                         f"roc_histogram, and ap_from_histogram(..., key='logit') reads it")
    if n and (h < 1 or w < 1):
        raise ValueError(f'empty planes: {tuple(scores.shape)}')
    if h * w > 2 ** 31 - 1:
        raise ValueError(f'planes of {h} x {w} pixels are too large: a block counts in 32 bits')
    _lib.require_gpu()
    if not scores.is_cuda:
        raise ValueError('expected fp32 scores (N,C,H,W) on the device')
    return scores.contiguous(), n, c, h, w  # (a view of a larger buffer at any element offset is read in place)


@torch.no_grad()
def score_histogram(scores: torch.Tensor, target: torch.Tensor, extent=None, bits: int = AP_BITS,
                    per_image: bool = False, per_class: bool = False) -> torch.Tensor:
    """fp32 scores (N,C,H,W) of a head of 2..255 classes on the device, read as they stand -- ``predict(scores=True)``
    writes them, any values in [0, 1] will do -- and a uint8 target (N,H,W) -> int64 CUDA tensor (2, 2^bits): row 1 counts
    the pairs (pixel, class k) with target == k, row 0 all others, per score bin, summed over batch and classes (the
    micro histogram of the one-hot target); (C, 2, 2^bits) with ``per_class``, (N, 2, 2^bits) with ``per_image``,
    (N, C, 2, 2^bits) with both (cae_seg_score_hist; asynchronous on the current stream).  A pixel whose label is >= C
    is unlabelled and counted nowhere.  ``extent``: (N,2) integers (rows, cols): only the pixels y < rows, x < cols of
    each image are counted (values are clamped to the plane).  Histograms are exact and add; ``ap_from_histogram`` makes
    average precision and its curve of them."""
    bits = _check_ap_bits(bits)
    scores, n, c, h, w = _scores_arg(scores)
    dev = scores.device
    tgt = _target_arg(target, dev, n, h, w)
    ext = _extent_arg(extent, n, dev)
    shape = ((n,) if per_image else ()) + ((c,) if per_class else ()) + (2, 1 << bits)
    with torch.cuda.device(dev):
        if n == 0:
            return torch.zeros(shape, dtype=torch.int64, device=dev)
        L = _lib.lib()
        hist = torch.empty(shape, dtype=torch.int64, device=dev)
        ws = _workspace(L.cae_seg_score_workspace(n, c, h, w, bits), dev)
        _lib.check(L.cae_seg_score_hist(scores.data_ptr(), tgt.data_ptr(), _ptr(ext), n, c, h, w, bits,
                                        int(bool(per_image)), int(bool(per_class)), hist.data_ptr(), ws.data_ptr(),
                                        ws.numel() * 8, _lib.stream_ptr()))
    return hist


def ap_from_histogram(hist, key: str = 'score') -> Dict:
    """One histogram (2, B) of score_histogram -- a tile's, or the sum of many tiles' -- or an (M, 2, B) array of them
    (per image, per class), which is summed -> dict(precision, recall, thresholds, avg_prec, avg_prec_lo, avg_prec_hi,
    p, n); pure numpy on the host.  ``key='logit'``: a histogram of roc_histogram instead, with roc_bin_edges -- the
    sigmoid is monotone, so a one-class head has its average precision from the histogram it already has.

    Walking the non-empty bins from the top down, with TP, FP the totals above bin b, p_b and n_b its positives and
    negatives and P = sum p_b:  ``avg_prec`` = (1/P) sum_b p_b (TP + p_b) / (TP + FP + p_b + n_b), which is sklearn's
    ``average_precision_score`` of the scores snapped to their bins (the ties of a bin are one threshold).  The average
    precision of the unbinned scores lies in [``avg_prec_lo``, ``avg_prec_hi``], whatever the order and ties inside a bin:
    hi = (1/P) sum_b p_b (TP + p_b) / (TP + FP + p_b) (no negative of the bin above any of its positives, and the
    precision behind the i-th positive grows with i); lo = (1/P) sum_b [p_b - (FP + n_b) ln((T + p_b) / T)], T = TP + FP
    + n_b, the term p_b where T = 0 (all negatives of the bin above its positives: sum_i (TP + i) / (T + i) = p_b -
    (FP + n_b) sum_i 1 / (T + i), and the sum is below the integral of 1/x).  lo = hi = avg_prec where no negative lies
    in or above a bin with positives.  Terms are divided in Python integers (correctly rounded) and added with
    math.fsum: avg_prec and hi are within 2^-51 of their exact values, lo within 2^-49.  All NaN without positives.

    ``precision`` / ``recall``: as sklearn's ``precision_recall_curve`` returns them for the snapped scores, one point per
    non-empty bin in rising order of ``thresholds`` (the bins' lower edges e_j: ``score >= e_j``), then the end point
    (1, 0)."""
    import math
    if key not in ('score', 'logit'):
        raise ValueError(f"key must be 'score' or 'logit', got {key!r}")
    neg, pos, N, P, bits = _histogram_arg(hist, AP_BITS_RANGE if key == 'score' else ROC_BITS_RANGE)
    full = np.flatnonzero(neg + pos)  # the non-empty bins, rising
    edges = (score_bin_edges if key == 'score' else roc_bin_edges)(bits)
    thr = edges[full].astype(np.float64)
    if not P:
        nan = float('nan')
        return dict(precision=np.full(full.size + 1, nan), recall=np.full(full.size + 1, nan), thresholds=thr,
                    avg_prec=nan, avg_prec_lo=nan, avg_prec_hi=nan, p=P, n=N)
    precision, recall = np.ones(full.size + 1), np.zeros(full.size + 1)
    mid, low, high = [], [], []
    TP = FP = 0
    for i in range(full.size - 1, -1, -1):  # Python integers: a slide's p_b (TP + p_b) does not fit 64 bits
        pb, nb = int(pos[full[i]]), int(neg[full[i]])
        precision[i], recall[i] = (TP + pb) / (TP + FP + pb + nb), (TP + pb) / P
        if pb:
            T = TP + FP + nb
            mid.append(pb * (TP + pb) / (T + pb))
            high.append(pb * (TP + pb) / (TP + FP + pb))
            low.append(pb - (FP + nb) * math.log1p(pb / T) if T else float(pb))
        TP, FP = TP + pb, FP + nb
    return dict(precision=precision, recall=recall, thresholds=thr, avg_prec=math.fsum(mid) / P,
                avg_prec_lo=math.fsum(low) / P, avg_prec_hi=math.fsum(high) / P, p=P, n=N)


# ---- object-level results: connected objects of the target, their boxes' cover, weighted counts (csrc/cae_seg_objects.hip)
def _check_planes(n: int, h: int, w: int):
    if n and (h < 1 or w < 1):
        raise ValueError(f'empty planes: {n} x {h} x {w}')
    if 3 * min(h, w) > 65535 or h * w > 2 ** 31 - 1:
        raise ValueError(f'planes of {h} x {w} pixels are too large: the cover of a pixel is held in 16 bits '
                         f'(3 min(H, W) <= 65535) and a label in 32')


def _planes_arg(planes, dtype, what: str, check=_check_planes):
    """a tensor of this dtype, (N,H,W), on the device; its shape is judged (``check``) before a device is asked for
    -> (n, h, w)"""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 3 or planes.dtype != dtype:
        raise ValueError(f'expected {what} (N,H,W) on the device')
    n, h, w = planes.shape
    check(n, h, w)
    _lib.require_gpu()
    if not planes.is_cuda:
        raise ValueError(f'expected {what} (N,H,W) on the device')
    return n, h, w


def _extent_arg(extent, n: int, dev):
    """(N,2) integers (rows, cols), on the device as the int32 the library reads (clamped there to the plane), or None"""
    if extent is None:
        return None
    ext = extent if isinstance(extent, torch.Tensor) else torch.as_tensor(np.asarray(extent))
    if ext.is_floating_point() or ext.dtype == torch.bool or tuple(ext.shape) != (n, 2):
        raise ValueError(f'expected an extent of {n} x 2 integers (rows, cols), got {ext.dtype} {tuple(ext.shape)}')
    i32 = torch.iinfo(torch.int32)
    return ext.clamp(i32.min, i32.max).to(device=dev, dtype=torch.int32).contiguous()


@torch.no_grad()
def components(target: torch.Tensor, extent=None, by_value: bool = False):
    """uint8 label planes (N,H,W) on the device, read as they stand -> (labels (N,H,W) int32, n_objects (N,) int64):
    the 8-connected objects of every plane (cae_seg_components; asynchronous on the current stream).  Foreground is
    ``target > 0`` inside ``extent`` ((N,2) integers (rows, cols), clamped to the plane; None: whole planes); with
    ``by_value`` neighbours join only when their values are equal (skimage.measure.label of an integer image), otherwise
    all foreground counts as one value (the reference's one-class case).  A label is 0 on background, else 1 + the
    smallest row-major index of its object; objects never reach across planes."""
    n, h, w = _planes_arg(target, torch.uint8, 'uint8 label planes')
    dev = target.device
    ext = _extent_arg(extent, n, dev)
    tgt = target.contiguous()  # (a view of a larger buffer at any byte offset is read in place)
    with torch.cuda.device(dev):
        labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int64, device=dev)
        if n:
            L = _lib.lib()
            ws = _workspace(L.cae_seg_components_workspace(n, h, w), dev)
            _lib.check(L.cae_seg_components(tgt.data_ptr(), _ptr(ext), n, h, w, int(bool(by_value)), labels.data_ptr(),
                                            count.data_ptr(), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr()))
    return labels, count


@torch.no_grad()
def object_cover(labels: torch.Tensor, extent=None) -> torch.Tensor:
    """labels (N,H,W) int32 of ``components`` (and its ``extent``) -> cover (N,H,W) uint16 on the device: the number of
    objects whose box holds the pixel (cae_seg_object_cover; asynchronous on the current stream).  The box of an object
    is its rows and columns widened by one pixel on every side, clipped to the extent (test_cae_classifier.py:101-109).
    The reference concatenates the pixels of all boxes, so its object-level sums are the image-level sums weighted by
    this cover."""
    n, h, w = _planes_arg(labels, torch.int32, 'int32 labels')
    dev = labels.device
    ext = _extent_arg(extent, n, dev)
    lab = labels.contiguous()
    with torch.cuda.device(dev):
        cover = torch.empty((n, h, w), dtype=torch.uint16, device=dev)
        if n:
            L = _lib.lib()
            ws = _workspace(L.cae_seg_object_cover_workspace(n, h, w), dev)
            _lib.check(L.cae_seg_object_cover(lab.data_ptr(), _ptr(ext), n, h, w, cover.data_ptr(), ws.data_ptr(),
                                              ws.numel() * 8, _lib.stream_ptr()))
    return cover


MAX_DISTANCE_EDGE = 32768  # cae_seg_object_distances: 2 (edge - 1)^2 stays below 2^31 - 1


def _check_distance_planes(n: int, h: int, w: int):
    if n and (h < 1 or w < 1):
        raise ValueError(f'empty planes: {n} x {h} x {w}')
    if max(h, w) > MAX_DISTANCE_EDGE or h * w > 2 ** 31 - 1:
        raise ValueError(f'planes of {h} x {w} pixels are too large: a squared distance is held in 32 bits '
                         f'(H, W <= {MAX_DISTANCE_EDGE}, H W <= 2^31 - 1)')


@torch.no_grad()
def object_distances(labels: torch.Tensor) -> torch.Tensor:
    """labels (N,H,W) int32 of ``components`` (0 is background; only that the labels of two objects differ matters) ->
    d2 (N,2,H,W) int32 on the device (cae_seg_object_distances; asynchronous on the current stream): plane 0 the squared
    Euclidean distance to the nearest foreground pixel (0 on foreground), plane 1 the smallest squared distance to a
    pixel of another object than the one that gives plane 0; -1 where there is no such object.  Exact integers, the
    distances of the reference's ``WeightsDistances`` (one distance transform per object there, two passes here)."""
    n, h, w = _planes_arg(labels, torch.int32, 'int32 labels', _check_distance_planes)
    dev = labels.device
    lab = labels.contiguous()
    with torch.cuda.device(dev):
        d2 = torch.empty((n, 2, h, w), dtype=torch.int32, device=dev)
        if n:
            L = _lib.lib()
            ws = _workspace(L.cae_seg_object_distances_workspace(n, h, w), dev)
            _lib.check(L.cae_seg_object_distances(lab.data_ptr(), n, h, w, d2.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                  _lib.stream_ptr()))
    return d2


def _check_cover(cover, n: int, hw: int, dev) -> torch.Tensor:
    if not isinstance(cover, torch.Tensor) or cover.dtype != torch.uint16 or cover.numel() != n * hw:
        raise ValueError(f'expected a uint16 cover of {n} x {hw} weights')
    return cover.to(dev).contiguous()


@torch.no_grad()
def object_counts(logits: torch.Tensor, target: torch.Tensor, cover: torch.Tensor, threshold: float = 0.5,
                  threshold_on: str = 'scores', top_k: int = 5) -> torch.Tensor:
    """The counts of ``predict`` with every pixel counted ``cover`` times -> (N,6) int64 [tp, tn, fp, fn, p, tp_top] on
    the device (cae_seg_object_counts; asynchronous on the current stream).  logits (N,C,...) fp32 on the device, target
    and cover uint8 / uint16 of N x pixels entries; threshold, threshold_on and top_k as in ``predict``.  With the cover
    of ``object_cover`` these are the reference's object-level counts; any uint16 weights are summed exactly."""
    t = threshold_logit(threshold, threshold_on)  # ValueError before anything else
    top_k = _check_top_k(top_k)
    logits, n, c, _, hw = _logits_arg(logits)
    dev = logits.device
    tgt, cov = _target_arg(target, dev, n, hw), _check_cover(cover, n, hw, dev)
    with torch.cuda.device(dev):
        counts = torch.empty((n, len(COUNT_KEYS)), dtype=torch.int64, device=dev)
        if n:
            L = _lib.lib()
            ws = _workspace(L.cae_seg_object_counts_workspace(n, c, hw), dev)
            _lib.check(L.cae_seg_object_counts(logits.data_ptr(), tgt.data_ptr(), cov.data_ptr(), n, c, hw, t, top_k,
                                               counts.data_ptr(), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr()))
    return counts


@torch.no_grad()
def object_roc_histogram(logits: torch.Tensor, target: torch.Tensor, cover: torch.Tensor, extent=None,
                         bits: int = ROC_BITS, per_image: bool = False) -> torch.Tensor:
    """``roc_histogram`` with every pixel adding ``cover`` (uint16, N x H x W) instead of 1 (cae_seg_object_roc_hist;
    asynchronous on the current stream): with the cover of ``object_cover`` the histogram of the pixels of all object
    boxes.  Same arguments, layout and bins otherwise; ``roc_from_histogram`` takes it as it is."""
    return _roc_histogram(logits, target, cover, extent, bits, per_image)
