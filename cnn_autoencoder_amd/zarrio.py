"""Zarr-v2 tile I/O and the compress / decompress flows of the reference, without third-party deps.

The reference delegates tile I/O to dask + zarr (``src/compress.py:78-128``,
``src/decompress.py:48-96``): the image is rechunked to ``(patch, patch, 3)`` and written with
``compressor=codec``, so every chunk file is exactly ``codec.encode(chunk)``.  This module writes and
reads the same on-disk layout (zarr format 2, directory store):

    <store>/<group>/.zgroup                       {"zarr_format": 2}
    <store>/<group>/<array>/.zarray               shape, chunks, dtype, compressor config, fill_value, order "C",
                                                  filters null, dimension_separator "."
    <store>/<group>/<array>/<i>.<j>.<k>           one file per chunk = the codec's bytes of the FULL chunk shape
                                                  (edge chunks are padded with fill_value, as zarr does)

so an array written here opens with ``zarr.open`` once ``register_codecs()`` has run, and vice versa.
Chunks are coded in batches on the GPU (``encode_batch`` / ``decode_batch``) instead of one dask task per
chunk; with ``torch.distributed`` initialised every rank codes the contiguous tile block
``slide.tile_range(rank, world, n_tiles)`` and rank 0 writes the metadata.
"""
from __future__ import annotations

import json
import math
import os
import zlib
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

ZARR_FORMAT = 2


class _Raw:
    codec_id = None

    def encode(self, buf):
        return np.ascontiguousarray(buf).tobytes()

    def decode(self, buf, out=None):
        return np.frombuffer(bytes(buf), dtype=np.uint8)

    def get_config(self):
        return None


class Zlib:
    """numcodecs.Zlib-compatible codec (the reference writes decompressed images with Blosc/zlib-9,
    decompress.py:48; Blosc itself is a third-party library and is not reimplemented)."""
    codec_id = 'zlib'

    def __init__(self, level: int = 1):
        self.level = int(level)

    def encode(self, buf):
        return zlib.compress(np.ascontiguousarray(buf).tobytes(), self.level)

    def decode(self, buf, out=None):
        return np.frombuffer(zlib.decompress(bytes(buf)), dtype=np.uint8)

    def get_config(self):
        return dict(id=self.codec_id, level=self.level)

    @classmethod
    def from_config(cls, config):
        config = dict(config)
        config.pop('id', None)
        return cls(**config)


def get_codec(config: Optional[dict]):
    """compressor config of a .zarray -> codec object (numcodecs.get_codec for the ids this path uses)."""
    if config is None:
        return _Raw()
    cid = config.get('id')
    if cid == 'zlib':
        return Zlib.from_config(config)
    if cid in ('cae', 'cae_bn'):
        from .codec import ConvolutionalAutoencoder, ConvolutionalAutoencoderBottleneck
        cls = ConvolutionalAutoencoder if cid == 'cae' else ConvolutionalAutoencoderBottleneck
        return cls.from_config(config)
    raise ValueError(f'Codec {cid!r} not supported')


def _ensure_groups(store: str, path: str):
    os.makedirs(store, exist_ok=True)
    parts = [p for p in path.split('/') if p]
    cur = store
    for p in [None] + parts[:-1]:
        if p is not None:
            cur = os.path.join(cur, p)
            os.makedirs(cur, exist_ok=True)
        zg = os.path.join(cur, '.zgroup')
        if not os.path.exists(zg) and not os.path.exists(os.path.join(cur, '.zarray')):
            with open(zg, 'w') as f:
                json.dump({'zarr_format': ZARR_FORMAT}, f)


class ZarrArray:
    """One zarr-v2 array in a directory store."""

    def __init__(self, root: str, meta: dict, codec=None):
        self.root = root
        self.meta = meta
        self.shape = tuple(meta['shape'])
        self.chunks = tuple(meta['chunks'])
        self.dtype = np.dtype(meta['dtype'])
        self.sep = meta.get('dimension_separator', '.')
        self.fill_value = meta.get('fill_value', 0) or 0
        self.codec = codec if codec is not None else get_codec(meta.get('compressor'))

    # ---- construction ------------------------------------------------------------------------
    @classmethod
    def create(cls, store: str, component: str, shape, chunks, dtype, codec=None, fill_value=0,
               write_meta: bool = True) -> 'ZarrArray':
        root = os.path.join(store, component) if component else store
        compressor = codec.get_config() if codec is not None else None
        meta = dict(zarr_format=ZARR_FORMAT, shape=[int(s) for s in shape], chunks=[int(c) for c in chunks],
                    dtype=np.dtype(dtype).str, compressor=compressor, fill_value=fill_value, order='C',
                    filters=None, dimension_separator='.')
        try:
            text = json.dumps(meta, indent=4, sort_keys=True)
        except TypeError as e:  # e.g. a 'cae' codec built from an in-memory checkpoint dict
            raise ValueError(f'the codec configuration cannot be stored in .zarray metadata ({e}): build the codec '
                             'from a checkpoint PATH when writing a store') from e
        # every rank creates the directories it writes chunk files into (a rank may finish its first batch before the
        # metadata writer has run); only the metadata writer touches the .zgroup / .zarray files
        if root is not None:
            os.makedirs(root, exist_ok=True)
        if write_meta:
            _ensure_groups(store, component)
            with open(os.path.join(root, '.zarray'), 'w') as f:
                f.write(text)
        return cls(root, meta, codec=codec if codec is not None else _Raw())

    @classmethod
    def open(cls, store: str, component: str = '', codec=None) -> 'ZarrArray':
        root = os.path.join(store, component) if component else store
        with open(os.path.join(root, '.zarray')) as f:
            meta = json.load(f)
        if meta.get('zarr_format') != ZARR_FORMAT:
            raise ValueError('only zarr format 2 is supported')
        if meta.get('filters'):
            raise ValueError('filters are not supported')
        if meta.get('order', 'C') != 'C':
            raise ValueError('only C order is supported')
        return cls(root, meta, codec=codec)

    # ---- attributes (.zattrs) ----------------------------------------------------------------
    @property
    def attrs(self) -> dict:
        """the array's user attributes: the JSON object of its .zattrs file, {} where there is none"""
        p = os.path.join(self.root, '.zattrs')
        if not os.path.exists(p):
            return {}
        with open(p) as f:
            return json.load(f)

    def write_attrs(self, attrs: dict):
        with open(os.path.join(self.root, '.zattrs'), 'w') as f:
            json.dump(dict(attrs), f, indent=4, sort_keys=True)

    @property
    def is_sparse(self) -> bool:
        """written by compress_image with a mask or a fill value (the attribute 'sparse'): chunks without a file are
        meant, and the slide drivers leave them out; in any other array they take a missing chunk file for damage"""
        return 'sparse' in self.attrs

    # ---- chunk grid --------------------------------------------------------------------------
    @property
    def grid(self) -> Tuple[int, ...]:
        return tuple(int(math.ceil(s / c)) for s, c in zip(self.shape, self.chunks))

    def chunk_indices(self) -> List[Tuple[int, ...]]:
        """All chunk coordinates in C (raster) order -- the tile order the slide driver shards."""
        return [tuple(int(v) for v in idx) for idx in np.ndindex(*self.grid)]

    def chunk_path(self, idx: Sequence[int]) -> str:
        return os.path.join(self.root, self.sep.join(str(int(i)) for i in idx))

    def chunk_slices(self, idx: Sequence[int]):
        return tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, self.chunks, self.shape))

    # ---- chunk I/O ---------------------------------------------------------------------------
    def pad_chunk(self, data: np.ndarray) -> np.ndarray:
        """Edge chunks are stored at the full chunk shape, padded with fill_value (zarr v2)."""
        if tuple(data.shape) == self.chunks:
            return np.ascontiguousarray(data, dtype=self.dtype)
        full = np.full(self.chunks, self.fill_value, dtype=self.dtype)
        full[tuple(slice(0, s) for s in data.shape)] = data
        return full

    def write_chunk_bytes(self, idx, cdata: bytes):
        with open(self.chunk_path(idx), 'wb') as f:
            f.write(cdata)

    def read_chunk_bytes(self, idx) -> Optional[bytes]:
        p = self.chunk_path(idx)
        if not os.path.exists(p):
            return None
        with open(p, 'rb') as f:
            return f.read()

    def write_chunk(self, idx, data: np.ndarray):
        self.write_chunk_bytes(idx, self.codec.encode(self.pad_chunk(data)))

    def read_chunk(self, idx) -> np.ndarray:
        cdata = self.read_chunk_bytes(idx)
        if cdata is None:
            return np.full(self.chunks, self.fill_value, dtype=self.dtype)
        out = np.asarray(self.codec.decode(cdata))
        return np.ascontiguousarray(out).view(self.dtype).reshape(self.chunks) if out.dtype != self.dtype \
            else out.reshape(self.chunks)

    def __setitem__(self, key, value):
        if key != slice(None) and key is not Ellipsis:
            raise NotImplementedError('only whole-array assignment is supported')
        value = np.asarray(value)
        if tuple(value.shape) != self.shape:
            raise ValueError(f'shape mismatch {value.shape} vs {self.shape}')
        for idx in self.chunk_indices():
            self.write_chunk(idx, value[self.chunk_slices(idx)])

    # ---- region reads ------------------------------------------------------------------------
    def normalize_key(self, key) -> List[Tuple[int, int, bool]]:
        """numpy basic indexing with step 1 -> per dimension (start, stop, is_integer), bounds clipped as numpy does.
        Integers, slices, one Ellipsis, negative bounds, fewer keys than dimensions; anything else raises (zarr's
        wording where zarr has one)."""
        keys = list(key) if isinstance(key, tuple) else [key]
        if sum(1 for k in keys if k is Ellipsis) > 1:
            raise IndexError("an index can only have a single ellipsis ('...')")
        n_given = sum(1 for k in keys if k is not Ellipsis)
        if n_given > len(self.shape):
            raise IndexError(f'too many indices for array; expected {len(self.shape)}, got {n_given}')
        if any(k is Ellipsis for k in keys):
            at = [k is Ellipsis for k in keys].index(True)
            keys[at:at + 1] = [slice(None)] * (len(self.shape) - n_given)
        keys += [slice(None)] * (len(self.shape) - len(keys))
        out = []
        for k, n in zip(keys, self.shape):
            if isinstance(k, slice):
                if k.step not in (None, 1):
                    raise NotImplementedError('only slices with step 1 are supported')
                start, stop, _ = k.indices(n)  # raises TypeError on non-integer bounds, as numpy does
                out.append((start, max(start, stop), False))
            elif isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_)):
                i = int(k)
                if i < -n or i >= n:
                    raise IndexError(f'index out of bounds for dimension with length {n}')
                i += n if i < 0 else 0
                out.append((i, i + 1, True))
            else:
                raise IndexError('unsupported selection item for basic indexing; expected integer or slice, got '
                                 f'{type(k)!r}')
        return out

    def _gather(self, sel, cshape, fetch) -> np.ndarray:
        """The region `sel` (normalize_key form, in the coordinates of an array whose chunks have shape `cshape`) from
        the chunks it touches, each fetched once: fetch(list of chunk indices) yields their arrays in order."""
        out = np.empty(tuple(b - a for a, b, _ in sel), dtype=self.dtype)
        squeeze = tuple(slice(None) if not is_int else 0 for _, _, is_int in sel)
        if out.size:
            touched = [tuple(int(v) for v in i) for i in np.ndindex(*[(b - 1) // c - a // c + 1
                                                                      for (a, b, _), c in zip(sel, cshape)])]
            touched = [tuple(i + a // c for i, (a, _, _), c in zip(idx, sel, cshape)) for idx in touched]
            for idx, chunk in zip(touched, fetch(touched)):
                src, dst = [], []
                for i, c, (a, b, _) in zip(idx, cshape, sel):
                    lo, hi = max(a, i * c), min(b, (i + 1) * c)
                    src.append(slice(lo - i * c, hi - i * c))
                    dst.append(slice(lo - a, hi - a))
                out[tuple(dst)] = chunk[tuple(src)]
        return out[squeeze]

    def __getitem__(self, key) -> np.ndarray:
        """Region read: numpy basic indexing with step 1 (see normalize_key).  Only the chunks the key touches are read
        and decoded, each once; a missing chunk file reads as fill_value."""
        return self._gather(self.normalize_key(key), self.chunks, lambda idxs: (self.read_chunk(i) for i in idxs))

    def read_region(self, key, scale: int = 0, batch_tiles: int = 32, coder: str = 'host') -> np.ndarray:
        """``self[key]`` at 1 / 2^scale of the resolution; `key` is in full-resolution coordinates.  The scale-s image
        of the array is the mosaic of its chunks' scale-s tiles; the result is rows floor(y0 / 2^s) : ceil(y1 / 2^s) of
        that mosaic, likewise for columns, channel keys as given.  The touched chunks of a 'cae' array are decoded in
        batches of `batch_tiles` (SlideCoder.decompress_batches: range decoder on `coder`, synthesis stopped at the
        level); scale > 0 needs such an array (and colour layers: multiscale_analysis=True)."""
        from .codec import ConvolutionalAutoencoder
        from .entropy import check_coder
        check_coder(coder)
        if isinstance(scale, bool) or int(scale) != scale or scale < 0:
            raise ValueError(f'scale must be a non-negative integer, got {scale!r}')
        scale = int(scale)
        sel = self.normalize_key(key)
        if not isinstance(self.codec, ConvolutionalAutoencoder):
            if scale > 0:
                raise ValueError("scale > 0 needs an array whose codec is 'cae'")
            return self[key]
        import struct
        f = 2 ** scale
        ph, pw = self.chunks[0], self.chunks[1]
        if len(self.shape) != 3 or ph % f or pw % f:
            raise ValueError(f'chunks {self.chunks} cannot be read at scale {scale}')
        def scaled(d, a, b, is_int):
            if d >= 2:
                return a, b, is_int
            if is_int:  # the pixel of the scaled image that holds it
                return a // f, a // f + 1, True
            return a // f, (max(a // f, -(-b // f)) if b > a else a // f), False
        sel = [scaled(d, *t) for d, t in enumerate(sel)]
        cshape = (ph // f, pw // f, self.chunks[2])

        def fetch(idxs):
            from . import slide
            sc = self.__dict__.setdefault('_slide_coders', {}).get(coder)
            if sc is None:
                sc = self._slide_coders[coder] = slide.SlideCoder(self.codec, coder=coder)
            bufs = {i: self.read_chunk_bytes(i) for i in idxs}
            have = [i for i in idxs if bufs[i] is not None]
            for i in have:
                if struct.unpack('>QQ', bufs[i][:16]) != (ph, pw):
                    raise ValueError('chunk header does not match the chunk shape')
            groups = list(_batches(have, batch_tiles))
            stream = sc.decompress_batches(([bufs[i][16:] for i in g] for g in groups), ph, pw, to_host=True,
                                           scale=scale)
            done = {}
            pending = iter(idxs)
            for g, rec in zip(groups, stream):  # rec: pinned ring buffer, copied out before the generator advances
                for i, tile in zip(g, rec):
                    done[i] = tile
                for i in pending:
                    yield done.pop(i) if bufs[i] is not None else np.full(cshape, self.fill_value, self.dtype)
                    if i == g[-1]:
                        break
            for i in pending:  # missing chunks behind the last decoded one
                yield np.full(cshape, self.fill_value, self.dtype)
        return self._gather(sel, cshape, fetch)


# ---- the reference's compress / decompress flows ---------------------------------------------------

def _rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


def _barrier():
    """All ranks have written their chunk files (the store is complete when compress_image returns)."""
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.barrier()
    except ImportError:
        pass


def _batches(items: Sequence, n: int) -> Iterable[Sequence]:
    for i in range(0, len(items), n):
        yield items[i:i + n]


def _sparse_plan(image, patch_size, keep, fill_value, max_fill_rmse, batch_tiles, rank, world):
    """Pass 1 of a sparse compress_image -> (the chunk indices of this rank that get no file, the fill value, the
    'sparse' attribute of the array).  `keep`: (grid rows, grid columns) bool, the chunks the mask keeps; the others are
    the candidates.  This rank's candidates go to the device in batches of `batch_tiles` padded chunks, their byte
    histograms over the real (rows, cols) come back, and fill value, rescues and the exact squared error follow on the
    host; the sums over the ranks are integer all-reduces.  With a given fill value and no guard nothing is uploaded."""
    import torch
    from . import slide, tissue
    h, w, c = image.shape
    src = ZarrArray(None, dict(shape=[h, w, c], chunks=[patch_size, patch_size, c], dtype='|u1'), codec=_Raw())
    tiles = src.chunk_indices()
    lo, hi = slide.tile_range(rank, world, len(tiles))
    cand = [idx for idx in tiles[lo:hi] if not keep[idx[0], idx[1]]]
    account = dict(tiles=len(tiles), kept=int(np.count_nonzero(keep)), rescued=0, skipped=len(tiles) - int(np.count_nonzero(keep)),
                   skipped_samples=None, skipped_sse=None)
    if fill_value is not None and max_fill_rmse is None:
        return set(cand), int(fill_value), dict(account, fill_value=int(fill_value))
    # two pinned staging buffers: the host fills one while the copy engine empties the other; a chunk's real part is
    # copied once and what lies beyond it is never counted, so nothing is padded; the histograms come back in one copy
    stage = [torch.empty((batch_tiles, patch_size, patch_size, c), dtype=torch.uint8).pin_memory() for _ in range(2)] if cand else []
    sent = [None, None]
    parts = []
    for k, group in enumerate(_batches(cand, batch_tiles)):
        pin = stage[k % 2]
        if sent[k % 2] is not None:
            sent[k % 2].synchronize()
        real = []
        for t, idx in enumerate(group):
            part = image[src.chunk_slices(idx)]
            pin[t, :part.shape[0], :part.shape[1]] = torch.from_numpy(part)
            real.append(part.shape[:2])
        batch = pin[:len(group)].to('cuda', non_blocking=True)
        sent[k % 2] = torch.cuda.Event()
        sent[k % 2].record()
        parts.append(tissue.tile_histograms(batch, real))
    hist = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 256), dtype=np.int64)
    if fill_value is None:
        total = slide.reduce_histogram(torch.from_numpy(hist.sum(axis=0)).cuda())
        fill_value = tissue.fill_from_histogram(total)[0]
    fill_value = int(fill_value)
    sse, samples = tissue.fill_sse(hist, fill_value), hist.sum(axis=1)
    if max_fill_rmse is None:
        rescue = np.zeros(len(cand), dtype=bool)
    else:
        rescue = sse.astype(np.float64) / np.maximum(samples, 1).astype(np.float64) > float(max_fill_rmse) ** 2
    mine = [int(np.count_nonzero(rescue)), int(np.count_nonzero(~rescue)), int(samples[~rescue].sum()),
            int(sse[~rescue].sum())]
    rescued, n_skipped, skipped_samples, skipped_sse = (int(v) for v in slide.reduce_histogram(
        torch.tensor(mine, dtype=torch.int64, device='cuda')).cpu())
    account.update(fill_value=fill_value, rescued=rescued, skipped=n_skipped, skipped_samples=skipped_samples,
                   skipped_sse=skipped_sse)
    return {idx for idx, r in zip(cand, rescue) if not r}, fill_value, account


def compress_image(codec: str, checkpoint, image: np.ndarray, output_filename: str, patch_size: int = 512,
                   data_group: str = '0/0', save_as_bottleneck: bool = False, gpu: bool = True,
                   batch_tiles: int = 32, coder: str = 'host', mask=None, mask_scale: Optional[float] = None,
                   fill_value: Optional[int] = None, max_fill_rmse: Optional[float] = None) -> ZarrArray:
    """compress.py:29-128 for an in-memory (H, W, C) uint8 image: rechunk to (patch, patch, C) and write a
    zarr array whose chunks are ``codec`` bitstreams.  codec: 'CAE' | 'Zlib' | 'None' (the reference's
    'Blosc' / 'Jpeg*' names are other libraries' codecs and raise ValueError here).  coder: where the range coder of
    the CAE codecs runs, 'host' or 'device' (same chunk bytes).

    Sparse stores ('CAE' pixel arrays only; without ``mask`` and ``fill_value`` nothing below applies and the store is
    what it always was).  ``mask`` (Y, X) at ``mask_scale`` mask pixels per image pixel, as tissue.tissue_mask and
    tissue.mask_zarr make it: the chunks that ``tissue.mask_tiles`` does not keep are candidates for skipping.  A skipped
    chunk has no file -- a stale one is removed -- and reads as the array's ``fill_value`` (zarr v2), which also pads the
    edge chunks.
    Pass 1 looks at this rank's candidates on the device (tissue.tile_histograms over each chunk's real pixels, batches of
    ``batch_tiles``): ``fill_value`` None takes the value with the least squared error over all candidates of all ranks
    (tissue.fill_from_histogram of the histograms' sum, slide.reduce_histogram), else an integer in 0..255 is taken as
    given.  ``max_fill_rmse``: a candidate whose squared error against the fill value per sample is above its square
    (float64) is rescued, i.e. coded like a kept chunk -- a pen mark, faint tissue the mask missed.  With a given
    ``fill_value`` and no ``max_fill_rmse`` no candidate is looked at or uploaded.
    Rank 0 writes ``.zattrs['sparse'] = dict(fill_value, tiles, kept, rescued, skipped, skipped_samples, skipped_sse)``,
    sums over all ranks: ``kept`` chunks the mask keeps, ``skipped_sse`` the exact integer squared error of the skipped
    chunks' real samples against the fill value (both ``skipped_*`` None where pass 1 did not run).  The squared error of
    the whole slide is ``skipped_sse`` plus the coded chunks' (slide.slide_summary's ``sse`` column), over all samples."""
    from . import slide
    from .entropy import check_coder
    check_coder(coder)
    from .codec import (ConvolutionalAutoencoder, ConvolutionalAutoencoderBottleneck, _module,
                        autoencoder_from_state_dict)
    image = np.asarray(image)
    if image.ndim != 3 or image.dtype != np.uint8:
        raise ValueError(f'expected a (H, W, C) uint8 image, got {image.dtype} {image.shape}')
    if not len(data_group):
        data_group = '0/0'
    h, w, c = image.shape
    rank, world = _rank_world()
    sparse = mask is not None or fill_value is not None
    if mask is None and (mask_scale is not None or max_fill_rmse is not None):
        raise ValueError('mask_scale and max_fill_rmse need a mask')
    if sparse:
        if 'CAE' not in codec or save_as_bottleneck:
            raise ValueError("a mask or a fill_value needs the 'CAE' pixel codec (no save_as_bottleneck, 'Zlib' or 'None')")
        if mask is not None and mask_scale is None:
            raise ValueError('a mask needs its mask_scale (mask pixels per image pixel)')
        if fill_value is not None and (isinstance(fill_value, (bool, np.bool_)) or not isinstance(
                fill_value, (int, np.integer)) or not 0 <= int(fill_value) <= 255):
            raise ValueError(f'fill_value is an integer in 0..255, got {fill_value!r}')
        if max_fill_rmse is not None and not (isinstance(max_fill_rmse, (int, float, np.integer, np.floating))
                                              and not isinstance(max_fill_rmse, bool) and max_fill_rmse >= 0):
            raise ValueError(f'max_fill_rmse is a number >= 0, got {max_fill_rmse!r}')
        if not 1 <= c <= 4:
            raise ValueError(f'a sparse store needs 1 to 4 channels, got {c}')
        keep = np.ones((-(-h // patch_size), -(-w // patch_size)), dtype=bool)
        if mask is not None:
            from . import tissue
            keep = tissue.mask_tiles(mask, mask_scale, image.shape, (patch_size, patch_size))
    if 'CAE' in codec and not save_as_bottleneck and not isinstance(checkpoint, str):
        # the 'cae' codec persists its checkpoint PATH in the .zarray metadata (_autoencoders.py:532): fail before
        # the model is built, not when the metadata is written
        raise ValueError("codec 'CAE' stores the checkpoint path in the array metadata: pass a path, not a dict")

    if 'CAE' in codec and save_as_bottleneck:
        import torch
        model = autoencoder_from_state_dict(checkpoint=checkpoint, gpu=gpu, train=False)
        fe = _module(model['fact_ent'])
        enc = _module(model['encoder'])
        level = len(enc.analysis_track)
        compressor = ConvolutionalAutoencoderBottleneck(channels_bn=fe.channels, fact_ent=fe, gpu=gpu)
        lat = int(math.ceil(patch_size / 2 ** level))
        gy, gx = int(math.ceil(h / patch_size)), int(math.ceil(w / patch_size))
        # latent array: per tile ceil(patch / 2^L) rows/cols (compress.py:103-107)
        z = ZarrArray.create(output_filename, data_group, (gy * lat, gx * lat, fe.channels), (lat, lat, fe.channels),
                             np.float32, codec=compressor, write_meta=rank == 0)
        src = ZarrArray(None, dict(shape=[h, w, c], chunks=[patch_size, patch_size, c], dtype='|u1'), codec=_Raw())
        tiles = src.chunk_indices()
        lo, hi = slide.tile_range(rank, world, len(tiles))
        for group in _batches(tiles[lo:hi], batch_tiles):
            batch = np.stack([src.pad_chunk(image[src.chunk_slices(i)]) for i in group])
            with torch.no_grad():
                y = enc.forward_u8(torch.from_numpy(batch).cuda())
                strings = fe.compress(y, coder=coder)
            for idx, s in zip(group, strings):
                import struct
                z.write_chunk_bytes(idx, struct.pack('>QQ', y.shape[2], y.shape[3]) + s)
        _barrier()
        return z

    if 'CAE' in codec:
        compressor = ConvolutionalAutoencoder(checkpoint=checkpoint, gpu=gpu)
    elif 'Zlib' in codec:
        compressor = Zlib(level=9)
    elif 'None' in codec:
        compressor = None
    else:
        raise ValueError('Codec %s not supported' % codec)
    skipped, account = set(), None
    if sparse:
        skipped, fill_value, account = _sparse_plan(image, patch_size, keep, fill_value, max_fill_rmse, batch_tiles,
                                                    rank, world)
    z = ZarrArray.create(output_filename, data_group, (h, w, c), (patch_size, patch_size, c), np.uint8,
                         codec=compressor, write_meta=rank == 0, **(dict(fill_value=fill_value) if sparse else {}))
    tiles = z.chunk_indices()
    lo, hi = slide.tile_range(rank, world, len(tiles))
    if isinstance(compressor, ConvolutionalAutoencoder):
        # pipelined: the GPU analyses the next batches while a host worker range-encodes and this thread writes files
        import struct
        for idx in tiles[lo:hi]:
            if idx in skipped and os.path.exists(z.chunk_path(idx)):  # a skipped chunk is a chunk without a file
                os.remove(z.chunk_path(idx))
        groups = list(_batches([i for i in tiles[lo:hi] if i not in skipped], batch_tiles))
        sc = slide.SlideCoder(compressor, coder=coder)
        stream = sc.compress_batches(np.stack([z.pad_chunk(image[z.chunk_slices(i)]) for i in g]) for g in groups)
        head = struct.pack('>QQ', patch_size, patch_size)  # chunk = '>QQ'(h, w) + rANS payload (_autoencoders.py:553-555)
        for group, payloads in zip(groups, stream):
            for idx, payload in zip(group, payloads):
                z.write_chunk_bytes(idx, head + payload)
        if sparse and rank == 0:
            z.write_attrs(dict(z.attrs, sparse=account))
        _barrier()
        return z
    for idx in tiles[lo:hi]:
        z.write_chunk(idx, image[z.chunk_slices(idx)])
    _barrier()
    return z


def decompress_image(input_filename: str, data_group: str = '0/0', checkpoint=None, gpu: bool = True,
                     batch_tiles: int = 32, coder: str = 'host', roi=None, scale: int = 0) -> np.ndarray:
    """decompress.py:40-96: open the zarr (chunk decode = the stored codec), and when `checkpoint` is given the
    array holds 'cae_bn' latents that the decoder turns back into pixels (decompress.py:61-79).  coder: 'host' or
    'device' range decoder of the 'cae' chunks.
    roi = (y0, y1, x0, x1), full-resolution pixels: the reference's ROI flow (decompress.py:49-59, parse_roi applied
    before anything is decoded) -- only the chunks under the rectangle are read and decoded.  scale = s: the image at
    1 / 2^s of the resolution (ZarrArray.read_region: rows floor(y0 / 2^s) : ceil(y1 / 2^s) of the mosaic of scale-s
    tiles); needs a 'cae' array or the 'cae_bn' + checkpoint branch, and a model with colour layers.
    The chunks a sparse store (``ZarrArray.is_sparse``) has no file for are not decoded: their part of the result is the
    array's fill_value, at any scale.  A full read of any other 'cae' store raises ValueError at a missing chunk file."""
    from .entropy import check_coder
    check_coder(coder)
    from .codec import ConvolutionalAutoencoder, _module, autoencoder_from_state_dict
    z = ZarrArray.open(input_filename, data_group)
    if isinstance(scale, bool) or int(scale) != scale or scale < 0:
        raise ValueError(f'scale must be a non-negative integer, got {scale!r}')
    scale = int(scale)
    if roi is not None:
        y0, y1, x0, x1 = (int(v) for v in roi)
        if not (0 <= y0 <= y1 and 0 <= x0 <= x1):
            raise ValueError(f'roi must be (y0, y1, x0, x1) with 0 <= y0 <= y1 and 0 <= x0 <= x1, got {tuple(roi)}')
    if checkpoint is None or (isinstance(checkpoint, str) and not len(checkpoint)):
        if roi is not None or scale:
            key = Ellipsis if roi is None else (slice(y0, y1), slice(x0, x1))
            return z.read_region(key, scale=scale, batch_tiles=batch_tiles, coder=coder)
        if isinstance(z.codec, ConvolutionalAutoencoder):
            # pipelined: a host worker range-decodes the next batches while the GPU synthesises
            import struct
            from . import slide
            out = np.empty(z.shape, dtype=z.dtype)
            present = z.chunk_indices()
            if z.is_sparse:  # the chunks without a file are not decoded: their part of the image is the fill value
                out[...] = z.fill_value
                present = [i for i in present if os.path.exists(z.chunk_path(i))]
            groups = list(_batches(present, batch_tiles))
            ph, pw = z.chunks[0], z.chunks[1]

            def payloads(group):
                bufs = [z.read_chunk_bytes(i) for i in group]
                if any(b is None for b in bufs):
                    raise ValueError('missing chunk file')
                for b in bufs:
                    if struct.unpack('>QQ', b[:16]) != (ph, pw):
                        raise ValueError('chunk header does not match the chunk shape')
                return [b[16:] for b in bufs]

            sc = slide.SlideCoder(z.codec, coder=coder)
            stream = sc.decompress_batches((payloads(g) for g in groups), ph, pw, to_host=True)
            for group, rec in zip(groups, stream):  # rec: pinned ring buffer, copied out right away
                for idx, chunk in zip(group, rec):
                    sl = z.chunk_slices(idx)
                    out[sl] = chunk[tuple(slice(0, s.stop - s.start) for s in sl)]
            return out
        return z[:]
    import torch
    model = autoencoder_from_state_dict(checkpoint=checkpoint, gpu=gpu, train=False)
    dec = _module(model['decoder'])
    scale = dec._check_scale(scale)
    up = 2 ** (dec.rec_level - scale)  # pixels of the result per latent element
    ly, lx = z.chunks[0], z.chunks[1]
    gy, gx = z.grid[0], z.grid[1]
    if roi is None:
        ty0, ty1, tx0, tx1 = 0, gy, 0, gx
    else:  # the tiles under the rectangle, and only their latent chunks
        full = 2 ** dec.rec_level
        y1, x1 = min(y1, gy * ly * full), min(x1, gx * lx * full)
        y0, x0 = min(y0, y1), min(x0, x1)
        ty0, tx0 = y0 // (ly * full), x0 // (lx * full)
        ty1, tx1 = max(ty0, -(-y1 // (ly * full))), max(tx0, -(-x1 // (lx * full)))
    # (ny*lat, nx*lat, C) float32 latents of those tiles, decoded by the 'cae_bn' codec
    lat = z[ty0 * ly:ty1 * ly, tx0 * lx:tx1 * lx]
    out = np.empty((lat.shape[0] * up, lat.shape[1] * up, dec._dims[0]), dtype=np.uint8)
    idxs = [(i, j, 0) for i in range(ty1 - ty0) for j in range(tx1 - tx0)]
    for group in _batches(idxs, batch_tiles):
        batch = np.stack([lat[i * ly:(i + 1) * ly, j * lx:(j + 1) * lx] for i, j, _ in group])
        with torch.no_grad():
            y_q = torch.from_numpy(batch).permute(0, 3, 1, 2).contiguous().cuda()
            rec = (dec.forward_scale_u8(y_q, scale) if scale else dec.forward_u8(y_q)).cpu().numpy()
        for (i, j, _), tile in zip(group, rec):
            out[i * ly * up:(i + 1) * ly * up, j * lx * up:(j + 1) * lx * up] = tile
    if roi is None:
        return out
    f = 2 ** scale
    oy, ox = ty0 * ly * up, tx0 * lx * up
    return np.ascontiguousarray(out[y0 // f - oy:max(y0 // f, -(-y1 // f)) - oy, x0 // f - ox:max(x0 // f, -(-x1 // f)) - ox])


def segment_image(input_filename: str, seg_model, output_filename: str, data_group: str = '0/0', checkpoint=None,
                  target_group: Optional[str] = None, batch_tiles: int = 4, threshold: float = 0.5,
                  threshold_on: str = 'scores', top_k: int = 5, scores: bool = False, coder: str = 'host',
                  roc_bits: Optional[int] = None, object_level: bool = False, ap_bits: Optional[int] = None) -> Dict:
    """The reference's segmentation harness on a compressed slide (test_cae_classifier.py:46-55 and its metrics), without
    decoding a pixel to the host: the chunk bytes of the 'cae'-coded array ``data_group`` of ``input_filename`` go through
    SlideCoder.segment_batches (range decoder on ``coder``, synthesis track, the head ``seg_model``, cae_seg_predict)
    and the class map is written to ``output_filename``:

        class/0/0    (H, W), '|b1' for one class ('|u1' otherwise), chunks (patch, patch), Zlib(9)
        scores/0/0   (C, H, W) float32, chunks (C, patch, patch), Zlib(9)            -- with ``scores``

    ``checkpoint``: the codec's checkpoint, instead of the path stored in the array's metadata.  With
    ``torch.distributed`` initialised every rank segments the tile block ``slide.tile_range(rank, world, n_tiles)`` and
    rank 0 writes the metadata, as compress_image does.
    ``target_group``: a (H, W) (or (H, W, 1)) uint8 label array of the input store, read tile by tile.  The counts are
    made per chunk and cover the image's pixels only: the padding of an edge chunk is labelled so that the device
    counts can be corrected exactly on the host (several classes: label 255, wrong in tp and tp_top, then fp = fn =
    pixels - tp and p = pixels of the real part -- so a ragged image with a target needs at most 255 classes; one class:
    label 0, and the padding's share of tn and fp is taken off from the class map).
    ``roc_bits`` (8..14, segmenters.ROC_BITS = 14; needs a target and a one-class head): the slide's threshold-free
    results from logit histograms of 2^roc_bits bins per class (segmenters.roc_histogram over each tile's real pixels,
    summed on the device, then over the ranks: slide.reduce_histogram).  The result gains 'auc', 'auc_slack' (the AUC of the
    unbinned logits lies inside auc +- auc_slack) and 'roc' (segmenters.roc_from_histogram), and rank 0 writes the curve as
    the reference does (test_cae_classifier.py:356-364), float32 1-D arrays in one chunk, Zlib(9):

        image_level/fpr, image_level/tpr, image_level/thrsh (thresholds on the scores), image_level/thrsh_logit

    ``object_level`` (needs a target): the second half of the reference's harness (--compute-components-metrics,
    test_cae_classifier.py:97-157, 267-370) per tile: the connected objects of the tile's labels (by value for a head of
    several classes), their boxes, and the counts -- with ``roc_bits`` the histogram too -- over the pixels of all boxes
    (SlideCoder.segment_batches(object_level=True)).  Every tile's real size is its extent, so the padding of an edge
    chunk is in no object and no box.  The result gains 'object_level': segmenters.class_metrics of the summed
    object-level record plus 'n_objects' (the slide's sum), 'records' ((tiles, 6), all ranks) and, with ``roc_bits``,
    'auc', 'auc_slack' and 'roc'; rank 0 then writes object_level/fpr, tpr, thrsh and thrsh_logit as above.  An object cut
    by a tile border counts as two.
    ``ap_bits`` (8..14, segmenters.AP_BITS = 14; needs a target): the slide's average precision, the reference's avg_prec
    (utils/_metrics.py:90-92), from histograms of 2^ap_bits bins -- several classes: the micro histogram of the softmax
    scores (segmenters.score_histogram); one class: the logit histogram -- over each tile's real pixels, summed on the
    device, then over the ranks (SlideCoder.segment_batches(ap_bits=...), slide.reduce_histogram).  The result gains
    'avg_prec', 'avg_prec_lo', 'avg_prec_hi' (the average precision of the unbinned scores lies between the last two) and
    'pr' (segmenters.ap_from_histogram), and rank 0 writes image_level/precision, image_level/recall and
    image_level/pr_thrsh (one threshold fewer than points; on the scores, or for one class on the logits) as above.

    A sparse store (compress_image with a mask; ``ZarrArray.is_sparse``): the chunks without a file are not run and get no
    class/0/0 or scores/0/0 chunk -- their fill 0 is the background class -- and the result gains 'skipped_tiles' (this
    rank's).  With a target the record of such a chunk is made on the host from its labels with the prediction "background
    everywhere": one class, tn = the count of target == 0 and fn = p = the count of target > 0; several classes, tp =
    tp_top = the count of target == 0, fp = fn = pixels - tp, p = pixels.  ``roc_bits``, ``ap_bits`` and ``object_level``
    raise ValueError there: a skipped chunk has no logit.  In any other store a missing chunk file raises ValueError.

    -> segmenters.class_metrics of the slide's summed record, plus
    'records': the (tiles, 6) int64 per-tile records of all ranks in tile order (slide.gather_counts), 'tiles' and
    'head_fp32_repeats' (this rank's); without a target only the last two."""
    import struct
    import torch
    from . import segmenters, slide
    from .codec import ConvolutionalAutoencoder, _module
    from .entropy import check_coder
    check_coder(coder)
    if object_level and target_group is None:
        raise ValueError('object_level needs a target_group: the objects are those of the labels')
    codec = None
    if checkpoint is not None and not (isinstance(checkpoint, str) and not len(checkpoint)):
        codec = ConvolutionalAutoencoder(checkpoint=checkpoint)
    z = ZarrArray.open(input_filename, data_group, codec=codec)
    if not isinstance(z.codec, ConvolutionalAutoencoder) or len(z.shape) != 3:
        raise ValueError("segment_image needs a (H, W, C) array whose codec is 'cae'")
    seg = _module(seg_model)
    H, W = z.shape[0], z.shape[1]
    ph, pw = z.chunks[0], z.chunks[1]
    C = seg._num_classes
    rank, world = _rank_world()
    tz = None
    if target_group is not None:
        tz = ZarrArray.open(input_filename, target_group)
        if tuple(tz.shape[:2]) != (H, W) or tz.dtype != np.uint8 or int(np.prod(tz.shape[2:])) != 1:
            raise ValueError(f'the target must be a ({H}, {W}) uint8 array, got {tz.dtype} {tz.shape}')
    if tz is not None and C > 255 and (H % ph or W % pw):
        raise ValueError('a target on an image that is no multiple of its chunks needs at most 255 classes (label 255 '
                         'marks the padding of the edge chunks)')
    if roc_bits is not None:
        if tz is None or C != 1:
            raise ValueError('roc_bits needs a target_group and a one-class head')
        roc_bits = segmenters._check_roc_bits(roc_bits)
    if ap_bits is not None:
        if tz is None:
            raise ValueError('ap_bits needs a target_group')
        if C > 255:
            raise ValueError(f'ap_bits takes heads of up to 255 classes, this one has {C}')
        ap_bits = segmenters._check_ap_bits(ap_bits)
    sparse = z.is_sparse
    if sparse and (roc_bits is not None or ap_bits is not None or object_level):
        raise ValueError('roc_bits, ap_bits and object_level are not available on a sparse store: a skipped chunk has '
                         'no logit')
    sc = slide.SlideCoder(z.codec, coder=coder)
    zc = ZarrArray.create(output_filename, 'class/0/0', (H, W), (ph, pw), np.bool_ if C == 1 else np.uint8,
                          codec=Zlib(9), write_meta=rank == 0)
    zs = ZarrArray.create(output_filename, 'scores/0/0', (C, H, W), (C, ph, pw), np.float32, codec=Zlib(9),
                          write_meta=rank == 0) if scores else None
    tiles = z.chunk_indices()
    lo, hi = slide.tile_range(rank, world, len(tiles))
    run = tiles[lo:hi]
    if sparse:  # the chunks without a file are not run: their class is the fill 0 of class/0/0, the background
        run = [i for i in run if os.path.exists(z.chunk_path(i))]
    groups = list(_batches(run, batch_tiles))
    # the real pixels (rows, cols) of every tile: an edge chunk is padded beyond them, and the padding is in no histogram
    sizes = [[(min(ph, H - i * ph), min(pw, W - j * pw)) for i, j, _ in g] for g in groups]

    def chunks(group):
        bufs = [z.read_chunk_bytes(i) for i in group]
        if any(b is None for b in bufs):
            raise ValueError('missing chunk file')
        return bufs

    def labels(group):
        out = np.full((len(group), ph, pw), 255 if C > 1 else 0, dtype=np.uint8)
        for t, (i, j, _) in enumerate(group):
            part = tz[i * ph:min((i + 1) * ph, H), j * pw:min((j + 1) * pw, W)]
            part = part.reshape(part.shape[0], part.shape[1])
            out[t, :part.shape[0], :part.shape[1]] = part
        return out

    stream = sc.segment_batches((chunks(g) for g in groups), ph, pw, seg,
                                targets=None if tz is None else (labels(g) for g in groups), threshold=threshold,
                                threshold_on=threshold_on, top_k=top_k, scores=scores, to_host=True, roc_bits=roc_bits,
                                extents=(np.array(s, dtype=np.int32).reshape(-1, 2) for s in sizes)
                                if roc_bits is not None or ap_bits is not None or object_level else None,
                                object_level=bool(object_level), ap_bits=ap_bits)
    records, obj_records, obj_numbers = [], [], []
    hists = {}  # 'roc_hist', 'object_roc_hist', 'ap_hist' -> this rank's sum, on the device
    # res['cls']: pinned ring buffer, written out before the generator advances
    for group, real, res in zip(groups, sizes, stream):
        for key in ('roc_hist', 'object_roc_hist', 'ap_hist'):
            if key in res:
                hists[key] = res[key] + hists.get(key, 0)
        if object_level:
            obj_records.append(torch.from_numpy(np.array(res['object_counts'], dtype=np.int64)))
            obj_numbers.append(torch.from_numpy(np.array(res['n_objects'], dtype=np.int64)))
        for t, ((i, j, _), (ch, cw)) in enumerate(zip(group, real)):
            zc.write_chunk((i, j), res['cls'][t, :ch, :cw].astype(zc.dtype))
            if zs is not None:
                zs.write_chunk((0, i, j), res['scores'][t, :, :ch, :cw])
        if res['counts'] is not None:
            rec = np.array(res['counts'], dtype=np.int64)
            for t, (ch, cw) in enumerate(real):
                if ch * cw == ph * pw:
                    continue
                if C > 1:  # the padding (label 255) is in neither tp nor tp_top
                    rec[t, 1:5] = (0, ch * cw - rec[t, 0], ch * cw - rec[t, 0], ch * cw)
                else:  # the padding (label 0) is tn where the class map is off and fp where it is on
                    pad_on = int(np.count_nonzero(res['cls'][t])) - int(np.count_nonzero(res['cls'][t, :ch, :cw]))
                    rec[t, 1] -= ph * pw - ch * cw - pad_on
                    rec[t, 2] -= pad_on
            records.append(torch.from_numpy(rec))
    out = dict(tiles=hi - lo, head_fp32_repeats=sc.timers.get('head_fp32_repeats', 0))
    if sparse:
        out['skipped_tiles'] = (hi - lo) - len(run)
    if tz is not None and len(run) < hi - lo:
        # a skipped chunk's record, made here from its labels: the prediction is background everywhere
        def background(idx):
            part = tz[idx[0] * ph:min((idx[0] + 1) * ph, H), idx[1] * pw:min((idx[1] + 1) * pw, W)]
            px, zero = int(part.size), int(np.count_nonzero(part == 0))
            return (0, zero, 0, px - zero, px - zero, 0) if C == 1 else (zero, 0, px - zero, px - zero, px, zero)

        done = dict(zip(run, torch.cat(records).numpy())) if records else {}
        rows = [done[i] if i in done else background(i) for i in tiles[lo:hi]]  # in tile order, as ever
        records = [torch.from_numpy(np.array(rows, dtype=np.int64).reshape(-1, slide.COUNTS_WIDTH))]

    def gathered(parts):  # this rank's (tiles, 6) records -> those of all ranks, in tile order
        local = torch.cat(parts) if parts else torch.zeros((0, slide.COUNTS_WIDTH), dtype=torch.int64)
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_backend() == 'nccl':
                local = local.cuda()
        except ImportError:
            pass
        return slide.gather_counts(local).cpu().numpy()

    def curve(group, hist, into):  # this rank's histogram (None: a rank without tiles) -> the slide's curve and AUC
        if hist is None:
            hist = torch.zeros((2, 1 << roc_bits), dtype=torch.int64, device='cuda')
        roc = segmenters.roc_from_histogram(slide.reduce_histogram(hist))
        into.update(auc=roc['auc'], auc_slack=roc['auc_slack'], roc=roc)
        for name, key in (('fpr', 'fpr'), ('tpr', 'tpr'), ('thrsh', 'score_thresholds'), ('thrsh_logit', 'thresholds')):
            v = roc[key].astype(np.float32)
            if rank == 0:
                ZarrArray.create(output_filename, f'{group}/{name}', v.shape, v.shape, np.float32, codec=Zlib(9))[:] = v

    if tz is not None:
        allrec = gathered(records)
        out.update(segmenters.class_metrics(allrec.sum(axis=0), multiclass=C > 1), records=allrec)
    if object_level:
        objrec = gathered(obj_records)
        # this rank's number of objects, summed over the ranks as the histograms are (an int64 all_reduce)
        numbers = torch.tensor([sum(int(v.sum()) for v in obj_numbers)], dtype=torch.int64, device='cuda')
        obj = dict(segmenters.class_metrics(objrec.sum(axis=0), multiclass=C > 1), records=objrec,
                   n_objects=int(slide.reduce_histogram(numbers)[0]))
        if roc_bits is not None:
            curve('object_level', hists.get('object_roc_hist'), obj)
        out['object_level'] = obj
    if roc_bits is not None:
        curve('image_level', hists.get('roc_hist'), out)
    if ap_bits is not None:
        hist = hists.get('ap_hist')
        if hist is None:  # a rank without tiles
            hist = torch.zeros((2, 1 << ap_bits), dtype=torch.int64, device='cuda')
        pr = segmenters.ap_from_histogram(slide.reduce_histogram(hist), key='score' if C > 1 else 'logit')
        out.update(avg_prec=pr['avg_prec'], avg_prec_lo=pr['avg_prec_lo'], avg_prec_hi=pr['avg_prec_hi'], pr=pr)
        for name, key in (('precision', 'precision'), ('recall', 'recall'), ('pr_thrsh', 'thresholds')):
            v = pr[key].astype(np.float32)
            if rank == 0 and v.size:  # (no labelled pixel at all: no threshold)
                ZarrArray.create(output_filename, f'image_level/{name}', v.shape, v.shape, np.float32, codec=Zlib(9))[:] = v
    _barrier()
    return out
