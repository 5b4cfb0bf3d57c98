"""The tissue mask of a slide on the device (csrc/cae_mask.hip), and what is built on it.

The reference's ``scripts/compute_mask.py`` takes the slide at about 1.25x and runs ``rgb2gray``, an Otsu threshold,
``remove_small_objects(256, connectivity=2)``, ``remove_small_holes(128 * 128)`` and ``binary_dilation(disk(16))`` over it;
its datasets then draw patches inside that mask (``--mask-group``).  Here:

    downscale      box average of a uint8 image on the device (cae_mask_downscale)
    tissue_mask    the five steps on the device; only 2 KB of counts per plane visit the host (for the threshold)
    otsu_threshold the threshold from 256 counts and their edges, on the host in float64
    mask_zarr      a store's image -> its mask under masks/0/0, with the attribute 'scale'
    mask_tiles     which chunks of an array a mask touches: what the samplers' ``mask_group`` keeps
    tile_histograms       exact byte histograms of tiles on the device (cae_tile_byte_hist, csrc/cae_tiles.hip): the look
                          zarrio.compress_image takes at the chunks a mask does not touch before it skips them
    fill_from_histogram, fill_sse   the fill value with the least squared error and that error, exact, on the host

The contract is stated in numpy / scipy terms ("Tissue mask"); parity with skimage's own functions is unpinned.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from .segmenters import MAX_DISTANCE_EDGE, _check_planes, _extent_arg, _workspace, object_distances

MAX_FACTOR = 64
BINS = 256


def _check_mask_planes(n: int, h: int, w: int):
    _check_planes(n, h, w)
    if max(h, w) > MAX_DISTANCE_EDGE:
        raise ValueError(f'planes of {h} x {w} pixels are too large: a squared distance is held in 32 bits '
                         f'(H, W <= {MAX_DISTANCE_EDGE})')


def _images_arg(img, channels=None):
    """uint8 (H,W,C) or (N,H,W,C), host or device -> ((N,H,W,C) on the device, contiguous; had a batch dimension)"""
    t = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img))
    if t.dtype != torch.uint8 or t.dim() not in (3, 4):
        raise ValueError(f'expected a uint8 image (H,W,C) or (N,H,W,C), got {t.dtype} {tuple(t.shape)}')
    batched = t.dim() == 4
    if not batched:
        t = t[None]
    n, h, w, c = t.shape
    if channels is not None and c != channels:
        raise ValueError(f'expected {channels} channels, got {c}')
    if not 1 <= c <= 4:
        raise ValueError(f'expected 1 to 4 channels, got {c}')
    if n and (h < 1 or w < 1):
        raise ValueError(f'empty images: {n} x {h} x {w}')
    if h * w > 2 ** 31 - 1:
        raise ValueError(f'images of {h} x {w} pixels are too large')
    return t, batched


@torch.no_grad()
def downscale(img, f: int) -> torch.Tensor:
    """uint8 (H,W,C) or (N,H,W,C), host or device -> (..., ceil(H / f), ceil(W / f), C) uint8 on the device: the mean of
    every f x f block, ``(2 sum + count) // (2 count)`` in integers; a block on the lower or right edge covers only real
    pixels (cae_mask_downscale; asynchronous on the current stream).  1 <= f <= 64."""
    if isinstance(f, bool) or int(f) != f or not 1 <= f <= MAX_FACTOR:
        raise ValueError(f'the factor is an integer in 1..{MAX_FACTOR}, got {f!r}')
    f = int(f)
    t, batched = _images_arg(img)
    dev = _lib.require_gpu()
    t = t.to(dev)
    n, h, w, c = t.shape
    # a window of a larger image (dense pixels, rows and images any distance apart) is read where it stands
    if not (t.stride(3) == 1 and t.stride(2) == c and t.stride(1) >= w * c and (n < 2 or t.stride(0) >= h * t.stride(1))):
        t = t.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((n, -(-h // f), -(-w // f), c), dtype=torch.uint8, device=dev)
        if n:
            _lib.check(_lib.lib().cae_mask_downscale(t.data_ptr(), n, h, w, c, t.stride(1), max(t.stride(0), h * t.stride(1)),
                                                     f, out.data_ptr(), _lib.stream_ptr()))
    return out if batched else out[0]


def otsu_threshold(counts, edges) -> float:
    """256 counts and their 257 edges (numpy.histogram) -> Otsu's threshold as skimage.filters.threshold_otsu forms it,
    in float64: bin centres, cumulative class weights and means from both ends, the between-class variance
    ``w1[:-1] w2[1:] (m1[:-1] - m2[1:])^2`` and the centre of the first bin at which it is largest.  Host code."""
    counts = np.asarray(counts, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    if counts.ndim != 1 or counts.size < 2 or edges.shape != (counts.size + 1,) or (counts < 0).any():
        raise ValueError(f'expected non-negative counts of k >= 2 bins and their k + 1 edges, got {counts.shape} and '
                         f'{edges.shape}')
    centres = (edges[:-1] + edges[1:]) / 2
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    with np.errstate(invalid='ignore', divide='ignore'):
        m1 = np.cumsum(counts * centres) / w1
        m2 = (np.cumsum((counts * centres)[::-1]) / w2[::-1])[::-1]
        var12 = w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2
    if not np.isfinite(var12).any():
        raise ValueError('the counts are all in one bin')
    return float(centres[int(np.nanargmax(var12))])


@torch.no_grad()
def tissue_mask(img, min_size: int = 256, area_threshold: int = 16384, radius: int = 16, taps: bool = False):
    """uint8 (H,W,3) or (N,H,W,3), host or device -> bool (..., H, W) on the device; planes never mix.

    1. gray = (0.2125 r + 0.7154 g) + 0.0721 b in float64, r = R / 255.0, every operation rounded on its own;
    2. Otsu: the counts of ``numpy.histogram(gray, 256)`` on the device, the threshold from them on the host
       (``otsu_threshold``); a constant plane's threshold is its value;
    3. tissue = gray <= threshold;
    4. 8-connected objects of fewer than ``min_size`` pixels are cleared;
    5. 4-connected components of the complement of fewer than ``area_threshold`` pixels are set (one that touches the
       border like any other);
    6. dilation by the disk dx^2 + dy^2 <= radius^2: squared distance to the nearest set pixel <= radius^2.

    ``taps``: -> (mask, dict(gray, minmax, counts, thr, thresholded, objects, holes)) with the planes after steps 3, 4
    and 5 as uint8 (counts int64 (N,256) and thr float64 (N,) on the host; counts of a constant plane are zero)."""
    for name, v in (('min_size', min_size), ('area_threshold', area_threshold), ('radius', radius)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError(f'{name} is a non-negative integer, got {v!r}')
    if radius > 46340:
        raise ValueError(f'radius {radius}: its square leaves 32 bits')
    t, batched = _images_arg(img, channels=3)
    n, h, w, _ = t.shape
    _check_mask_planes(n, h, w)
    dev = _lib.require_gpu()
    t = t.to(dev).contiguous()
    hw = h * w
    L = _lib.lib() if n else None
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()
        gray = torch.empty((n, h, w), dtype=torch.float64, device=dev)
        minmax = torch.empty((n, 2), dtype=torch.float64, device=dev)
        plane = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        counts = np.zeros((n, BINS), dtype=np.int64)
        thr = np.zeros((n,), dtype=np.float64)
        tap = {}
        if n:
            _lib.check(L.cae_mask_gray(t.data_ptr(), n, hw, gray.data_ptr(), minmax.data_ptr(), st))
            lohi = minmax.cpu().numpy()
            edges = np.stack([np.linspace(lo, hi, BINS + 1) for lo, hi in lohi])
            varied = lohi[:, 0] != lohi[:, 1]
            if varied.any():
                edges_dev = torch.from_numpy(edges).to(dev)
                counts_dev = torch.empty((n, BINS), dtype=torch.int64, device=dev)
                ws = _workspace(L.cae_mask_hist_workspace(n, hw), dev)
                _lib.check(L.cae_mask_hist(gray.data_ptr(), edges_dev.data_ptr(), n, hw, counts_dev.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 8, st))
                counts = counts_dev.cpu().numpy()
                counts[~varied] = 0
            for i in range(n):
                thr[i] = otsu_threshold(counts[i], edges[i]) if varied[i] else lohi[i, 0]
            thr_dev = torch.from_numpy(thr).to(dev)
            _lib.check(L.cae_mask_threshold(gray.data_ptr(), thr_dev.data_ptr(), n, hw, plane.data_ptr(), st))
            if taps:
                tap['thresholded'] = plane.clone()
            labels = torch.empty((n, h, w), dtype=torch.int32, device=dev)
            wide = torch.empty((n, h, w), dtype=torch.int32, device=dev)
            ws = _workspace(max(L.cae_mask_label_workspace(n, h, w), L.cae_mask_area_workspace(n, h, w)), dev)
            for step, (conn, of_zero, least, value) in (('objects', (8, 0, int(min_size), 0)),
                                                        ('holes', (4, 1, int(area_threshold), 1))):
                _lib.check(L.cae_mask_label(plane.data_ptr(), n, h, w, conn, of_zero, labels.data_ptr(), ws.data_ptr(),
                                            ws.numel() * 8, st))
                _lib.check(L.cae_mask_area_filter(labels.data_ptr(), n, h, w, min(least, 2 ** 31 - 1), value, plane.data_ptr(),
                                                  wide.data_ptr() if step == 'holes' else None, ws.data_ptr(),
                                                  ws.numel() * 8, st))
                if taps:
                    tap[step] = plane.clone()
            d2 = object_distances(wide)
            _lib.check(L.cae_mask_within(d2.data_ptr(), n, hw, int(radius) ** 2, plane.data_ptr(), st))
        elif taps:
            tap.update(thresholded=plane.clone(), objects=plane.clone(), holes=plane.clone())
        mask = plane.view(torch.bool)
    if not batched:
        mask = mask[0]
    if not taps:
        return mask
    tap.update(gray=gray, minmax=minmax, counts=counts, thr=thr)
    return mask, tap


def mask_tiles(mask, scale: float, shape, chunks) -> np.ndarray:
    """Which chunks of an array of (Y, X) ``shape`` and ``chunks`` a mask at ``scale`` (mask pixels per array pixel)
    touches -> bool (grid rows, grid columns).  The footprint of the chunk with rows y0:y1 is the mask rows
    floor(y0 scale) : ceil(y1 scale), clipped to the mask; likewise columns; a chunk is kept if any pixel there is set."""
    mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    if mask.ndim != 2:
        raise ValueError(f'expected a (Y, X) mask, got {mask.shape}')
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f'scale {scale!r} is not finite and positive')
    (H, W), (ch, cw) = (int(v) for v in shape[:2]), (int(v) for v in chunks[:2])
    if min(H, W, ch, cw) < 1:
        raise ValueError(f'shape {tuple(shape)} / chunks {tuple(chunks)}')
    eps = 1e-9  # y scale of an exact product may land a rounding error beside its integer

    def span(a, b, most):
        return min(most, int(math.floor(a * scale + eps))), min(most, max(int(math.ceil(b * scale - eps)), 0))

    gy, gx = -(-H // ch), -(-W // cw)
    keep = np.zeros((gy, gx), dtype=bool)
    for i in range(gy):
        r0, r1 = span(i * ch, min((i + 1) * ch, H), mask.shape[0])
        for j in range(gx):
            c0, c1 = span(j * cw, min((j + 1) * cw, W), mask.shape[1])
            keep[i, j] = bool(mask[r0:r1, c0:c1].any())
    return keep


# ---- the look at background tiles: exact byte histograms, and the fill value and squared error they fix ----------------
@torch.no_grad()
def tile_histograms(tiles: torch.Tensor, extents=None) -> torch.Tensor:
    """uint8 tiles (N,H,W,C) on the device, contiguous, C <= 4, read where they stand (any byte address) -> int64 CUDA
    tensor (N, 256): how many samples of every tile hold each value (cae_tile_byte_hist, csrc/cae_tiles.hip; asynchronous on
    the current stream).  ``extents``: (N,2) integers (rows, cols): only the samples y < rows, x < cols of each tile are
    counted (values are clamped to the tile), so the padding of an edge chunk is in no histogram.  Counts are exact and
    add over tiles, batches and ranks; every row sums to rows cols C."""
    if not isinstance(tiles, torch.Tensor):
        raise ValueError(f'expected a uint8 tensor (N,H,W,C) on the device, got {type(tiles).__name__}')
    if tiles.dtype != torch.uint8 or tiles.dim() != 4:
        raise ValueError(f'expected uint8 tiles (N,H,W,C), got {tiles.dtype} {tuple(tiles.shape)}')
    n, h, w, c = tiles.shape
    if not 1 <= c <= 4:
        raise ValueError(f'expected 1 to 4 channels, got {c}')
    if n and (h < 1 or w < 1):
        raise ValueError(f'empty tiles: {n} x {h} x {w}')
    if not tiles.is_cuda:
        raise ValueError(f'expected tiles on the device, got them on {tiles.device}: there is no CPU path')
    if not tiles.is_contiguous():
        raise ValueError('expected contiguous tiles')
    dev = tiles.device
    ext = _extent_arg(extents, n, dev)
    with torch.cuda.device(dev):
        if n == 0:
            return torch.zeros((0, BINS), dtype=torch.int64, device=dev)
        L = _lib.lib()
        hist = torch.empty((n, BINS), dtype=torch.int64, device=dev)
        ws = _workspace(L.cae_tile_byte_hist_workspace(n, h, w, c), dev)
        _lib.check(L.cae_tile_byte_hist(tiles.data_ptr(), None if ext is None else ext.data_ptr(), n, h, w, c,
                                        hist.data_ptr(), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr()))
    return hist


def _counts(hist) -> np.ndarray:
    """integer histograms (..., 256), host or device -> the same as Python integers (an object array): no product or sum
    of them is rounded or wraps"""
    if isinstance(hist, torch.Tensor):
        hist = hist.detach().cpu().numpy()
    hist = np.asarray(hist)
    if hist.dtype.kind not in 'iuO' or hist.ndim not in (1, 2) or hist.shape[-1] != BINS:
        raise ValueError(f'expected integer histograms (256,) or (N, 256), got {hist.dtype} {hist.shape}')
    out = hist.astype(object)
    if any(v < 0 for v in out.ravel()):
        raise ValueError('a histogram holds a negative count')
    return out


def fill_from_histogram(hist):
    """Histograms (N, 256) of tile_histograms (or one, (256,)) -> (fill, sse): with cnt = their sum over the tiles, the f
    in 0..255 with the smallest sum_v cnt[v] (v - f)^2, the smallest such f on a tie, and that sum.  Python integers on the
    host: exact whatever the counts.  All counts zero: (0, 0)."""
    cnt = _counts(hist)
    if cnt.ndim == 2:
        cnt = cnt.sum(axis=0) if cnt.shape[0] else np.zeros(BINS, dtype=object)
    s0 = sum(int(k) for k in cnt)
    s1 = sum(int(k) * v for v, k in enumerate(cnt))
    s2 = sum(int(k) * v * v for v, k in enumerate(cnt))
    best = min(range(BINS), key=lambda f: (s2 - 2 * f * s1 + f * f * s0, f))
    return best, s2 - 2 * best * s1 + best * best * s0


def fill_sse(hist, fill: int) -> np.ndarray:
    """Histograms (N, 256) of tile_histograms and a fill value in 0..255 -> int64 (N,): sum_v hist[i][v] (v - fill)^2, the
    squared error of every tile against the fill value, exact (a sum beyond 2^63 - 1 is an OverflowError)."""
    if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255:
        raise ValueError(f'the fill value is an integer in 0..255, got {fill!r}')
    cnt = _counts(hist)
    if cnt.ndim != 2:
        raise ValueError(f'expected histograms (N, 256), got {cnt.shape}')
    weight = np.array([(v - int(fill)) ** 2 for v in range(BINS)], dtype=object)
    sums = [int(sum(row * weight)) for row in cnt]
    if any(s > np.iinfo(np.int64).max for s in sums):
        raise OverflowError('a squared error leaves 64 bits')
    return np.array(sums, dtype=np.int64).reshape(len(sums))


MASK_GROUP = 'masks/0/0'


@torch.no_grad()
def mask_zarr(input_filename: str, output_filename: Optional[str] = None, data_group: str = '0/0', factor: int = 32,
              batch_tiles: int = 16, coder: str = 'host', **mask_kwargs) -> np.ndarray:
    """The tissue mask of the (Y, X, 3) uint8 array ``data_group`` of a store, written to ``masks/0/0`` of
    ``output_filename`` (None: the input store) as '|b1', Zlib(9), with the attribute ``scale = 1 / factor``; returns it.
    The array is read chunk by chunk through ``ZarrArray`` -- the chunks of a 'cae' array through
    ``SlideCoder.decompress_batches``, whose tiles stay on the device -- and the real part of every chunk is reduced by
    ``downscale`` there; ``factor`` must divide the chunk edges.  ``tissue_mask(**mask_kwargs)`` then runs on the
    assembled image, which is 1 / factor^2 of the slide.  (The reference reads the magnification from the OME metadata;
    here the caller gives ``factor``.)"""
    import struct
    from .codec import ConvolutionalAutoencoder
    from .zarrio import ZarrArray, Zlib, _batches
    z = ZarrArray.open(input_filename, data_group)
    if len(z.shape) != 3 or z.shape[2] != 3 or z.chunks[2] != 3 or z.dtype != np.uint8:
        raise ValueError(f'expected a (Y, X, 3) uint8 array with whole pixels in a chunk, got {z.dtype} {z.shape} in chunks {z.chunks}')
    if isinstance(factor, bool) or int(factor) != factor or not 1 <= factor <= MAX_FACTOR:
        raise ValueError(f'the factor is an integer in 1..{MAX_FACTOR}, got {factor!r}')
    f = int(factor)
    H, W = z.shape[:2]
    ph, pw = z.chunks[:2]
    if ph % f or pw % f:
        raise ValueError(f'factor {f} does not divide the chunk edges {ph} x {pw}')
    dev = _lib.require_gpu()
    small = torch.empty((-(-H // f), -(-W // f), 3), dtype=torch.uint8, device=dev)
    groups = list(_batches(z.chunk_indices(), int(batch_tiles)))

    def place(group, tiles):
        """tiles (n, ph, pw, 3) on the device, padded: every chunk's real part, reduced, goes to its place"""
        real = [(min(ph, H - i * ph), min(pw, W - j * pw)) for i, j, _ in group]
        reduced = downscale(tiles, f)  # right for the whole chunks; a ragged one is reduced again from its real window
        for k, ((i, j, _), (rh, rw)) in enumerate(zip(group, real)):
            part = reduced[k] if (rh, rw) == (ph, pw) else downscale(tiles[k, :rh, :rw], f)
            small[i * (ph // f):i * (ph // f) + part.shape[0], j * (pw // f):j * (pw // f) + part.shape[1]] = part

    if isinstance(z.codec, ConvolutionalAutoencoder):
        from . import slide

        def payloads(group):
            bufs = [z.read_chunk_bytes(i) for i in group]
            if any(b is None for b in bufs):
                raise ValueError('missing chunk file')
            for b in bufs:
                if struct.unpack('>QQ', b[:16]) != (ph, pw):
                    raise ValueError('chunk header does not match the chunk shape')
            return [b[16:] for b in bufs]

        sc = slide.SlideCoder(z.codec, coder=coder)
        for group, rec in zip(groups, sc.decompress_batches((payloads(g) for g in groups), ph, pw, to_host=False)):
            place(group, rec)
    else:
        for group in groups:
            place(group, torch.from_numpy(np.stack([z.read_chunk(i) for i in group])).to(dev))
    mask = tissue_mask(small, **mask_kwargs).cpu().numpy()
    out = ZarrArray.create(output_filename if output_filename is not None else input_filename, MASK_GROUP, mask.shape,
                           mask.shape, np.bool_, codec=Zlib(9))
    out[:] = mask
    out.write_attrs({'scale': 1.0 / f})
    return mask
