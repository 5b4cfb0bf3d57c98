"""Yardstick of the MS-SSIM distortions: a torch-CPU restatement of ``pytorch_msssim.ms_ssim`` with win_size, win_sigma,
data_range and the dtype as parameters, differentiable by autograd, for (N, C, H, W) batches; and on top of it the padding
and window rule of the reference's ``DistMSSSIMLoss`` / ``DistMSSSIMPyramidLoss`` (``models/criteria/_ratedist.py:10-43,
66-107``).

``pytorch_msssim`` is absent from the machines this suite runs on, so parity with the package itself is unpinned, as for
the MS-SSIM metric: the formula is restated from the published implementation.  It is anchored to what is committed:
with (11, 1.5, 255), float32 and uint8 inputs it reproduces ``oracle.cae_oracle.ms_ssim_uint8``
(test_msssim_loss.py::test_anchor_to_committed_oracle).

A helper module, not a test file and not a conftest.
"""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(win_size, win_sigma, dtype=torch.float64):
    """_fspecial_gauss_1d"""
    coords = torch.arange(win_size, dtype=dtype) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    return g / g.sum()


def level_maps(X, Y, g, c1, c2):
    """one scale: the per-pixel (ssim map, cs map), each (N, C, H - win + 1, W - win + 1) in the dtype of X; the window
    applied separably without padding, dimension 2 first"""
    C = X.shape[1]
    k = g.to(X.dtype).view(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def gauss(t):
        return F.conv2d(F.conv2d(t, k.transpose(2, 3), groups=C), k, groups=C)

    mu1, mu2 = gauss(X), gauss(Y)
    s1, s2, s12 = gauss(X * X) - mu1 * mu1, gauss(Y * Y) - mu2 * mu2, gauss(X * Y) - mu1 * mu2
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim_map = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * cs_map
    return ssim_map, cs_map


def level(X, Y, g, c1, c2):
    """one scale: (ssim mean, cs mean) per (N, C) of level_maps"""
    ssim_map, cs_map = level_maps(X, Y, g, c1, c2)
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def pool(X):
    """the 2 x 2 average pooling between scales: zero padding of odd sizes, padded samples counted"""
    return F.avg_pool2d(X, kernel_size=2, padding=[s % 2 for s in X.shape[2:]])


def ms_ssim(X, Y, data_range=1.0, win_size=11, win_sigma=1.5, dtype=torch.float64, return_cs=False):
    """pytorch_msssim.ms_ssim(X, Y, data_range, size_average=True, win_size, win_sigma) computed in `dtype`"""
    X, Y = X.to(dtype), Y.to(dtype)
    assert min(X.shape[-2:]) > (win_size - 1) * 2 ** 4
    g = window(win_size, win_sigma, dtype)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mcs, cs_means = [], []
    for lvl in range(5):
        ssim_c, cs_c = level(X, Y, g, c1, c2)
        cs_means.append(cs_c)
        if lvl < 4:
            mcs.append(torch.relu(cs_c))
            X, Y = pool(X), pool(Y)
    vals = torch.stack(mcs + [torch.relu(ssim_c)], dim=0)
    out = torch.prod(vals ** torch.tensor(WEIGHTS, dtype=dtype).view(-1, 1, 1), dim=0).mean()
    return (out, torch.stack(cs_means, 0)) if return_cs else out


def loss_params(patch_size, scale=0):
    """(win_size, win_sigma, padding per side) of DistMSSSIMLoss(patch_size, scale)"""
    win = 11 - 2 * scale
    pad = (win - patch_size // 2 ** (scale + 4)) * 8
    return win, 1.5 / 2 ** scale, (pad if pad > 0 else 0)


def dist_msssim(x, x_r, patch_size, scale=0, normalize=False, dtype=torch.float64, return_cs=False):
    """DistMSSSIMLoss: 1 - ms_ssim(pad(x_r), pad(x))"""
    win, sigma, pad = loss_params(patch_size, scale)
    x, x_r = x.to(dtype), x_r.to(dtype)
    if pad:
        x, x_r = F.pad(x, (pad,) * 4), F.pad(x_r, (pad,) * 4)
    res = ms_ssim(x_r, x, 2.0 if normalize else 1.0, win, sigma, dtype, return_cs)
    return (1 - res[0], res[1]) if return_cs else 1 - res


def pyramid_down(x):
    """PyramidLossMixin.downsample_pyramid: 5 x 5 binomial blur / 256, zero padding 2, then bilinear x 0.5"""
    k1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=x.dtype)
    k = (k1[:, None] * k1[None, :] / 256.0).reshape(1, 1, 5, 5).repeat(x.size(1), 1, 1, 1)
    with torch.no_grad():
        return F.interpolate(F.conv2d(x, k, padding=2, groups=x.size(1)), scale_factor=0.5, mode='bilinear',
                             align_corners=False)


def dist_msssim_pyramid(x, x_r, patch_size, dtype=torch.float64):
    """DistMSSSIMPyramidLoss: level s of x_r against the s-times downsampled x under DistMSSSIMLoss(scale=s)"""
    x = x.to(dtype)
    dist = []
    for s, x_r_s in enumerate(x_r):
        dist.append(dist_msssim(x, x_r_s, patch_size, s, dtype=dtype))
        if s < len(x_r) - 1:
            x = pyramid_down(x)
    return dist


CASES = ((256, 0, 256), (256, 1, 128), (256, 2, 64), (256, 3, 32), (128, 0, 128), (192, 0, 192))  # (patch, scale, side)
SIGMAS = (0.02, 0.1)


def field(patch, scale, hw, n=2, c=3):
    """The inputs of the GPU cases: x = a smooth random field plus noise in [0, 1], and {sigma: x_r = x + sigma * noise}
    (not clamped) for the two noise levels.  For CASES x SIGMAS the float64 gradients are finite and every per-plane cs
    mean is >= 0.55 (>= 0.97 at sigma 0.02), so relu and the fractional power never meet zero."""
    gen = torch.Generator().manual_seed(patch + scale)
    base = F.interpolate(torch.rand(n, c, hw // 8 + 1, hw // 8 + 1, generator=gen), size=(hw, hw), mode='bilinear')
    x = (base + 0.05 * torch.randn(n, c, hw, hw, generator=gen)).clamp(0, 1)
    return x, {sigma: x + sigma * torch.randn(n, c, hw, hw, generator=gen) for sigma in SIGMAS}
