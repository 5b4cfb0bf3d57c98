"""Evaluation side of the reference's training objective (config 5's `valid` loop): the forward function of
``models/tasks/_taskutils.py:95-108`` and the rate / distortion terms of ``models/criteria`` -- ``RateLoss`` and
``DistMSELoss`` (``_ratedist.py:45-63``) assembled as ``GeneralLoss`` does (``_lossutils.py:54-72,100-109``):
``loss = lambda * 255^2 * MSE(x_r, x) + (-sum log2 p_y / (B H W))`` plus the reported ``entropy_loss``.

Under ``torch.no_grad()`` the analysis / synthesis tracks and the eval-mode density run on the inference kernels; with
autograd recording (``train.train_step``) the tracks switch to the training kernels with hand-written backward
(``train.py``) and the entropy model adds its uniform noise (train mode).  Classifier heads and penalty terms of the
reference are outside the hot path and not built; the segmentation head (``segmenters.JNet``, key ``'seg_model'``)
runs for inference only.  The multiscale objective
(``RateMultiscaleMSE``, ``DistMSEPyramidLoss`` of ``_ratedist.py:10-43, 88-93``) scores the colour layers of a
``multiscale_analysis`` decoder against a blurred, downsampled pyramid of the input (``pyramid_down``).

The MS-SSIM distortions (``RateMSSSIM``, ``RateMultiscaleMSSSIM``; ``DistMSSSIMLoss`` / ``DistMSSSIMPyramidLoss`` of
``_ratedist.py:66-107``) restate ``pytorch_msssim.ms_ssim`` (absent here: "parity unpinned", as the metric).  On GPU
tensors the five scales run on fused forward / backward kernels (``cae_t_msssim_level_fwd`` / ``_bwd``, csrc/
cae_msssim_train.hip); on CPU tensors, or with ``force_torch=True``, the same formula runs as torch ops under autograd.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Sequence, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


def setup_forward_func(enabled_modules: Sequence[str] = ('encoder', 'fact_ent', 'decoder')):
    """decorate_trainable_modules / forward_func of the reference for the modules of the hot path; disabled modules
    are identities exactly as there (`_taskutils.py:40-80`)."""
    enabled = set(enabled_modules)
    unknown = enabled - {'encoder', 'fact_ent', 'decoder', 'seg_model'}
    if unknown:
        raise NotImplementedError(f'modules outside the compression path are not built: {sorted(unknown)}')

    def forward_func(x, model) -> Dict:
        y = model['encoder'](x) if 'encoder' in enabled else x
        y_q, p_y = model['fact_ent'](y) if 'fact_ent' in enabled else (y, None)
        x_r, fx_brg = model['decoder'](y_q) if 'decoder' in enabled else (y_q, None)
        s_pred = s_aux_pred = None
        if 'seg_model' in enabled:
            # compressed-domain analysis beside the codec (`_taskutils.py:101-102`): inference only
            if torch.is_grad_enabled() and (x.requires_grad or any(
                    q.requires_grad for m in model.values() for q in m.parameters())):
                raise NotImplementedError("'seg_model' with autograd recording: training the segmentation head is not "
                                          'built; call forward_func under torch.no_grad()')
            s_pred, s_aux_pred = model['seg_model'](y_q, fx_brg=fx_brg)
        return dict(x_r=x_r, fx_brg=fx_brg, y=y, y_q=y_q, p_y=p_y, t_pred=None, t_aux_pred=None, s_pred=s_pred,
                    s_aux_pred=s_aux_pred)

    return forward_func


class RateLoss:
    """_ratedist.py:45-54."""

    def __init__(self, **kwargs):
        pass

    def __call__(self, x, p_y, **kwargs):
        rate_loss = -torch.sum(torch.log2(p_y)) / (x.size(0) * x.size(2) * x.size(3))
        return dict(rate_loss=rate_loss)


class DistMSELoss:
    """_ratedist.py:57-63."""

    def __init__(self, **kwargs):
        self._dist_loss = nn.MSELoss()

    def __call__(self, x, x_r, **kwargs):
        return dict(dist=[self._dist_loss(x_r[0], x.to(x_r[0].device))])


def pyramid_down(x: torch.Tensor) -> torch.Tensor:
    """One step of the reference's input pyramid (PyramidLossMixin.downsample_pyramid, _ratedist.py:10-31): depthwise 5 x 5
    binomial blur / 256 with zero padding 2, then bilinear x 0.5 (align_corners=False).  (n, c, h, w) -> (n, c, h/2, w/2).
    GPU tensors: one launch of cae_t_pyramid_down (the two steps fused as a stride-2 [1 5 10 10 5 1] / 32 filter); CPU
    tensors: the reference's torch formula."""
    if x.is_cuda:
        x = x.detach().float().contiguous()
        n, c, h, w = x.shape
        out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().cae_t_pyramid_down(x.data_ptr(), n, c, h, w, out.data_ptr(), _lib.stream_ptr()))
        return out
    k1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0])
    kernel = (k1[:, None] * k1[None, :] / 256.0).reshape(1, 1, 5, 5).repeat(x.size(1), 1, 1, 1)
    with torch.no_grad():
        x_dwn = F.conv2d(x, kernel.to(device=x.device, dtype=x.dtype), padding=2, groups=x.size(1))
        return F.interpolate(x_dwn, scale_factor=0.5, mode='bilinear', align_corners=False)


class DistMSEPyramidLoss:
    """_ratedist.py:10-43, 88-93: level s of x_r ([reconstruction, colour layer of half resolution, ...], as the
    Synthesizer returns it with multiscale_analysis) against `pyramid_down` applied s times to x; one MSE per level, at
    most compression_level of them."""

    def __init__(self, channels_org=3, compression_level=4, **kwargs):
        self.channels_org, self.levels = int(channels_org), int(compression_level)
        self._dist_loss = nn.MSELoss()

    def __call__(self, x, x_r, **kwargs):
        dist = []
        x_org = x.to(x_r[0].device) if x_r and x_r[0] is not None else x
        for s, x_r_s in enumerate(list(x_r)[:self.levels]):
            if x_r_s is None:
                raise ValueError(f'x_r[{s}] is None: the decoder was built without multiscale_analysis')
            dist.append(self._dist_loss(x_r_s, x_org.to(x_r_s.device)))
            if s < self.levels - 1:
                x_org = pyramid_down(x_org)
        return dict(dist=dist)


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _gauss_taps(win_size: int, win_sigma: float, dtype=torch.float32) -> torch.Tensor:
    """pytorch_msssim._fspecial_gauss_1d: normalised Gaussian taps, formed in `dtype`."""
    co = torch.arange(win_size, dtype=dtype) - win_size // 2
    g = torch.exp(-(co ** 2) / (2 * win_sigma ** 2))
    return g / g.sum()


def _pooled_size(s: int) -> int:
    return (s + 2 * (s % 2) - 2) // 2 + 1


def _msssim_levels_torch(X, Y, taps, c1, c2):
    """The five scales as torch ops (any device, the dtype of X) -> cs (5, N, C), ssim (N, C) of the last scale."""
    C = X.shape[1]
    g = taps.to(device=X.device, dtype=X.dtype).view(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def gauss(t):  # dimension 2 first, without padding
        return F.conv2d(F.conv2d(t, g.transpose(2, 3), groups=C), g, groups=C)

    cs, ssim_c = [], None
    for lvl in range(5):
        mu1, mu2 = gauss(X), gauss(Y)
        s1, s2, s12 = gauss(X * X) - mu1 * mu1, gauss(Y * Y) - mu2 * mu2, gauss(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
        ssim_map = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * cs_map
        cs.append(cs_map.flatten(2).mean(-1))
        ssim_c = ssim_map.flatten(2).mean(-1)
        if lvl < 4:
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    return torch.stack(cs, 0), ssim_c


class _MSSSIMLevels(torch.autograd.Function):
    """The five scales on the fused kernels: (X, Y) fp32 CUDA (N, C, H, W) -> cs (5, N, C), ssim (N, C), float64.
    Saves the two image pyramids (through save_for_backward: level 0 of X is X itself when it is contiguous, and an in-place
    change of it before the backward is then caught); the backward recomputes the local moments.  No gradient for Y."""

    @staticmethod
    def forward(ctx, X, Y, taps, c1, c2):
        L = _lib.lib()
        st = _lib.stream_ptr()
        n, c, h, w = X.shape
        planes = n * c
        win = len(taps)
        taps_c = (ctypes.c_double * win)(*taps)
        xs, ys, sizes = [X.contiguous()], [Y.float().contiguous()], [(h, w)]
        out = torch.empty((5, planes, 2), dtype=torch.float64, device=X.device)
        ws = torch.empty(2 * planes * (-(-(h - win + 1) // 32)) * (-(-(w - win + 1) // 32)), dtype=torch.float64,
                         device=X.device)
        for lvl in range(5):
            hh, ww = sizes[lvl]
            _lib.check(L.cae_t_msssim_level_fwd(xs[lvl].data_ptr(), ys[lvl].data_ptr(), planes, hh, ww, taps_c, win, c1, c2,
                                                out[lvl].data_ptr(), ws.data_ptr(), ws.numel(), st))
            if lvl < 4:
                h2, w2 = _pooled_size(hh), _pooled_size(ww)
                for seq in (xs, ys):
                    nxt = torch.empty((planes, h2, w2), dtype=torch.float32, device=X.device)
                    _lib.check(L.cae_avgpool2(seq[lvl].data_ptr(), planes, hh, ww, nxt.data_ptr(), st))
                    seq.append(nxt)
                sizes.append((h2, w2))
        ctx.save_for_backward(*xs, *ys)
        ctx.sizes, ctx.taps, ctx.c = sizes, taps, (c1, c2)
        return out[:, :, 1].reshape(5, n, c), out[4, :, 0].reshape(n, c)

    @staticmethod
    def backward(ctx, g_cs, g_ssim):
        L = _lib.lib()
        st = _lib.stream_ptr()
        saved, sizes, taps, (c1, c2) = ctx.saved_tensors, ctx.sizes, ctx.taps, ctx.c
        xs, ys = saved[:5], saved[5:]
        X = xs[0]
        n, c = g_ssim.shape
        h, w = sizes[0]
        planes = n * c
        win = len(taps)
        taps_c = (ctypes.c_double * win)(*taps)
        g_cs = g_cs.to(torch.float64).reshape(5, planes).contiguous()
        g_ssim = g_ssim.to(torch.float64).reshape(planes).contiguous()
        ws = torch.empty(3 * planes * (h - win + 1) * (w - win + 1), dtype=torch.float32, device=X.device)
        g = torch.zeros((planes,) + sizes[4], dtype=torch.float32, device=X.device)
        for lvl in range(4, -1, -1):  # coarsest first: the gradient of scale l = its own term + the pooled-back one of l + 1
            hh, ww = sizes[lvl]
            if lvl < 4:
                fine = torch.empty((planes, hh, ww), dtype=torch.float32, device=X.device)
                _lib.check(L.cae_t_avgpool2_bwd(g.data_ptr(), planes, hh, ww, fine.data_ptr(), st))
                g = fine
            _lib.check(L.cae_t_msssim_level_bwd(xs[lvl].data_ptr(), ys[lvl].data_ptr(), planes, hh, ww, taps_c, win, c1, c2,
                                                g_ssim.data_ptr() if lvl == 4 else None, g_cs[lvl].data_ptr(),
                                                g.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return g.reshape(n, c, h, w), None, None, None, None


def ms_ssim(X: torch.Tensor, Y: torch.Tensor, data_range: float = 1.0, win_size: int = 11, win_sigma: float = 1.5,
            force_torch: bool = False) -> torch.Tensor:
    """pytorch_msssim.ms_ssim(X, Y, data_range, size_average=True, win_size, win_sigma) for (N, C, H, W) images: five
    scales, weights MS_SSIM_WEIGHTS, K = (0.01, 0.03); the mean over N and C.  X is the reconstruction and carries the
    gradient; Y is the target and receives NONE (the training objective never needs it).  CUDA tensors: fp32 images, float64
    moments, maps and means on the fused kernels, a float64 result; CPU tensors, or any tensor with `force_torch`: torch ops in the
    dtype of X (differentiable in both arguments by autograd).  The combination of the per-scale means (relu, the weights
    as exponents, the product, the mean) is torch ops in both forms."""
    if X.shape != Y.shape or X.dim() != 4:
        raise ValueError(f'ms_ssim takes two (N, C, H, W) images of one shape, got {tuple(X.shape)} and {tuple(Y.shape)}')
    if win_size % 2 != 1:
        raise ValueError('Window size should be odd.')
    assert min(X.shape[-2:]) > (win_size - 1) * 2 ** 4, \
        'Image size should be larger than %d due to the 4 downsamplings in ms-ssim' % ((win_size - 1) * 2 ** 4)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    if X.is_cuda and not force_torch:
        if X.dtype != torch.float32:
            raise TypeError(f'the fused MS-SSIM kernels take float32 images, got {X.dtype}: cast, or pass force_torch=True')
        taps = [float(t) for t in _gauss_taps(win_size, win_sigma, torch.float64)]
        cs, ssim_c = _MSSSIMLevels.apply(X, Y.to(X.device), taps, c1, c2)
    else:
        cs, ssim_c = _msssim_levels_torch(X, Y.to(device=X.device, dtype=X.dtype), _gauss_taps(win_size, win_sigma, X.dtype),
                                          c1, c2)
    vals = torch.relu(torch.cat([cs[:4], ssim_c[None]], 0))
    weights = torch.tensor(MS_SSIM_WEIGHTS, dtype=vals.dtype, device=vals.device)
    return torch.prod(vals ** weights.view(-1, 1, 1), dim=0).mean()


class DistMSSSIMLoss:
    """_ratedist.py:66-90: dist = [1 - ms_ssim(x_r[0], x)] with the window of pyramid level `scale` (win_size 11 - 2 scale,
    sigma 1.5 / 2^scale) and zero padding of (win_size - patch_size // 2^(scale + 4)) * 8 pixels per side on both images
    when that is positive, which keeps the fifth scale larger than the window."""

    def __init__(self, patch_size, scale=0, normalize=False, force_torch=False, **kwargs):
        self.data_range = 2.0 if normalize else 1.0
        self.win_size = 11 - 2 * int(scale)
        self.win_sigma = 1.5 / 2 ** int(scale)
        pad = (self.win_size - int(patch_size) // 2 ** (int(scale) + 4)) * 8
        self.padding = pad if pad > 0 else 0
        self.force_torch = bool(force_torch)

    def __call__(self, x, x_r, **kwargs):
        x_rec = x_r[0]
        x = x.to(x_rec.device)
        if self.padding:
            x_rec, x = F.pad(x_rec, (self.padding,) * 4), F.pad(x, (self.padding,) * 4)
        return dict(dist=[1.0 - ms_ssim(x_rec, x, self.data_range, self.win_size, self.win_sigma, self.force_torch)])


class DistMSSSIMPyramidLoss:
    """_ratedist.py:10-43, 101-107: level s of x_r against `pyramid_down` applied s times to x, each under
    DistMSSSIMLoss(scale=s); at most compression_level levels."""

    def __init__(self, patch_size, channels_org=3, compression_level=4, normalize=False, force_torch=False, **kwargs):
        self.levels = int(compression_level)
        self._dist_loss = [DistMSSSIMLoss(patch_size, scale=s, normalize=normalize, force_torch=force_torch)
                           for s in range(self.levels)]

    def __call__(self, x, x_r, **kwargs):
        dist = []
        x_org = x.to(x_r[0].device) if x_r and x_r[0] is not None else x
        for s, x_r_s in enumerate(list(x_r)[:self.levels]):
            if x_r_s is None:
                raise ValueError(f'x_r[{s}] is None: the decoder was built without multiscale_analysis')
            dist.extend(self._dist_loss[s](x=x_org.to(x_r_s.device), x_r=[x_r_s])['dist'])
            if s < self.levels - 1:
                x_org = pyramid_down(x_org)
        return dict(dist=dist)


class GeneralLoss(nn.Module):
    """_lossutils.py:5-109 restricted to dist_loss_type='MSE' | 'MultiscaleMSE' | 'MSSSIM' | 'MultiscaleMSSSIM' | None and
    rate_loss_type='Rate' | None.  dist_loss = sum over zip(dist, distortion_lambda): a scalar lambda weights level 0
    only, as in the reference.  The distortions are multiplied by 255^2 for the MSE types only (_lossutils.py:19)."""

    def __init__(self, dist_loss_type='MSE', rate_loss_type='Rate', penalty_loss_type=None, class_loss_type=None,
                 distortion_lambda: Union[float, Sequence[float]] = 0.1, **kwargs):
        super().__init__()
        if (dist_loss_type not in (None, 'MSE', 'MultiscaleMSE', 'MSSSIM', 'MultiscaleMSSSIM')
                or rate_loss_type not in (None, 'Rate')):
            raise NotImplementedError('only the MSE / MS-SSIM distortions, their multiscale forms and the Rate term are built')
        if dist_loss_type and 'MSSSIM' in dist_loss_type and kwargs.get('patch_size') is None:
            raise NotImplementedError('the MS-SSIM distortions need patch_size (it sets their zero padding): pass patch_size=...')
        for name, v in (('penalty_loss_type', penalty_loss_type), ('class_loss_type', class_loss_type)):
            if v is not None and str(v).lower() != 'none':
                raise NotImplementedError(f'{name}={v!r} is outside the compression path')
        self.dist_loss = (None if not dist_loss_type else
                          DistMSEPyramidLoss(**kwargs) if dist_loss_type == 'MultiscaleMSE' else
                          DistMSSSIMPyramidLoss(**kwargs) if dist_loss_type == 'MultiscaleMSSSIM' else
                          DistMSSSIMLoss(**kwargs) if dist_loss_type == 'MSSSIM' else DistMSELoss())
        self.rate_loss = RateLoss() if rate_loss_type else None
        self._multiplier = 1 if dist_loss_type and 'MSSSIM' in dist_loss_type else 255 ** 2
        self._distortion_lambda = list(distortion_lambda) if isinstance(distortion_lambda, (list, tuple)) else [distortion_lambda]

    def forward(self, inputs, outputs, targets=None, net=None, **kwargs):
        loss_dict = {'loss': 0, 'channel_e': torch.LongTensor([-1])}
        if self.dist_loss is not None:
            loss_dict.update(self.dist_loss(x=inputs, x_r=outputs['x_r']))
            loss_dict['dist'] = [self._multiplier * d for d in loss_dict['dist']]
            loss_dict['dist_loss'] = sum(d * w for d, w in zip(loss_dict['dist'], self._distortion_lambda))
            loss_dict['loss'] = loss_dict['loss'] + loss_dict['dist_loss']
        if self.rate_loss is not None:
            loss_dict.update(self.rate_loss(x=inputs, p_y=outputs['p_y']))
            fe = net['fact_ent']
            loss_dict['entropy_loss'] = getattr(fe, 'module', fe).loss()
            loss_dict['loss'] = loss_dict['loss'] + loss_dict['rate_loss']
        return loss_dict


def setup_loss(criterion: str, **kwargs) -> GeneralLoss:
    """``models/criteria/_lossutils.py:112-151``: the criterion NAME selects the terms ('RateMSE' = the reference's
    default, ``utils/args/_critargs.py:42``).  Built: the Rate term, the MSE and MS-SSIM distortions and their multiscale
    pyramid forms ('RateMultiscaleMSE', 'RateMultiscaleMSSSIM': pass channels_org and compression_level).  The MS-SSIM
    distortions need patch_size, as DistMSSSIMLoss.__init__ of the reference does: without it they raise
    NotImplementedError.  The names of the terms outside the compression path (penalties, classification losses) raise."""
    name = criterion.lower()
    rate = 'Rate' if 'rate' in name else None
    if 'mse' in name:
        dist = 'MSE'
    elif 'msssim' in name or 'ms-ssim' in name:
        dist = 'MSSSIM'
        if kwargs.get('patch_size') is None:
            raise NotImplementedError(f'criterion {criterion!r}: the MS-SSIM distortion needs patch_size (it sets the zero '
                                      'padding of the images): pass patch_size=...')
    else:
        dist = None
    if 'multiscale' in name:
        if dist is None:
            raise NotImplementedError(f'criterion {criterion!r}: a multiscale term needs the MSE or MS-SSIM distortion')
        dist = 'Multiscale' + dist
    # (the reference tests `'pa' in name` / `'ce' in name` as plain substrings; those terms are not built here)
    for key in ('penalty', 'crossentropy', 'bce', 'weighted'):
        if key in name:
            raise NotImplementedError(f'criterion {criterion!r}: the {key} term is outside the compression hot path')
    return GeneralLoss(dist, rate, 'none', None, **kwargs)
