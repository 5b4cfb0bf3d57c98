"""Training input on the device: sample and augment patches out of a pool of uint8 tiles in HBM.

Stands where the reference's ``train_data`` / ``get_zarr_transform`` (utils/datasets/_augs.py:197-264, label_density == 0)
stand: ToTensor, AddGaussianNoise(0, 0.001), RandomCrop(pad_if_needed) or CenterCrop, Normalize(0.5, 0.5) and a bilinear
RandomRotation(30), but for a whole batch in one HIP kernel (``cae_t_sample_patches``, contract in include/cae_hip.h)
that writes the fp32 NCHW batch ``train.train_step`` takes.  The random draws (tile, offsets, angle) are host code with
torchvision's policies; the per-pixel work, the Gaussian noise included (a counter-based Philox4x32-10 stream), is the
kernel's.

``LabeledPatchSampler`` stands where the same transform stands with ``label_density == 2`` (_augs.py:52-82, 240-299):
image and pixel labels under one crop and one rotation, ``scipy.ndimage.rotate`` with reflected edges (spline order 4 on
the image, nearest neighbour on the mask), in ``cae_t_sample_labeled_patches``; its batches ``(x, t)`` are what
``seg_train.train_step`` takes.

``elastic_deform`` stands where ``RandomElasticDeformationInput`` / ``RandomElasticDeformationInputTarget`` stand
(_augs.py:26-49, 85-99; ``elastic_deformation=True``): a 3 x 3 grid of random displacements bent into a per-pixel field,
the image resampled through the cubic B-spline and the mask by its nearest neighbour (``cae_t_elastic_deform``).  Both
samplers apply it after their rotation with ``elastic_deformation=True``.

Under several ranks every rank builds its own sampler and passes ``draw`` / ``sample`` a generator seeded per rank (and
a per-rank ``seed`` for the noise): the sampler itself shares nothing between ranks.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

_M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def philox_normals(seed: int, sample: np.ndarray, pixel: np.ndarray) -> np.ndarray:
    """The four standard normals of the contract for every (sample index, patch pixel index) pair: Philox4x32-10 in
    exact integer arithmetic, Box-Muller in float64.  Returns float64 [..., 4].  (Host code: the values force_torch
    uploads.)"""
    c = [np.asarray(sample, dtype=np.uint64) & np.uint64(0xFFFFFFFF), np.asarray(pixel, dtype=np.uint64) & np.uint64(0xFFFFFFFF)]
    c[0], c[1] = np.broadcast_arrays(c[0], c[1])
    c += [np.zeros_like(c[0]), np.zeros_like(c[0])]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]  # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    u = [(w.astype(np.float64) + 0.5) * 2.0 ** -32 for w in c]
    out = np.empty(c[0].shape + (4,), dtype=np.float64)
    for pair in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[2 * pair]))
        out[..., 2 * pair] = r * np.cos(2.0 * np.pi * u[2 * pair + 1])
        out[..., 2 * pair + 1] = r * np.sin(2.0 * np.pi * u[2 * pair + 1])
    return out


def _zarr_tiles(stores, group: str, mask_group: Optional[str] = None):
    """Every chunk of the ``group`` array (Y, X, C uint8; or Y, X) of each store as one tile, padded to the chunk shape:
    ``(tiles, valid (rows, columns) per tile, [(Y, X) shape and chunks per store])``.  With ``mask_group`` only the
    chunks that the store's mask touches (``tissue.mask_tiles``; a bool or uint8 (Y', X') array with the attribute
    ``scale``, as ``tissue.mask_zarr`` writes it); ValueError if that leaves none."""
    from .zarrio import ZarrArray
    tiles, hw, shape, geometry = [], [], None, []
    for store in ([stores] if isinstance(stores, str) else stores):
        arr = ZarrArray.open(store, group)
        keep = None
        if mask_group is not None:
            from .tissue import mask_tiles
            marr = ZarrArray.open(store, mask_group)
            if 'scale' not in marr.attrs:
                raise ValueError(f"{store}: the mask {mask_group} has no 'scale' attribute")
            if len(marr.shape) != 2 or marr.dtype not in (np.dtype(np.bool_), np.dtype(np.uint8)):
                raise ValueError(f'{store}: expected a bool or uint8 (Y, X) mask, got {marr.dtype} {marr.shape}')
            keep = mask_tiles(marr[:], float(marr.attrs['scale']), arr.shape[:2], arr.chunks[:2])
        if len(arr.shape) not in (2, 3) or arr.dtype != np.uint8:
            raise ValueError(f'{store}: expected a uint8 (Y, X, C) or (Y, X) array, got {arr.dtype} {arr.shape}')
        if len(arr.shape) == 3 and arr.chunks[2] != arr.shape[2]:
            raise ValueError(f'{store}: chunks must hold all channels of a pixel')
        if shape is None:
            shape = arr.chunks
        elif arr.chunks != shape:
            raise ValueError(f'{store}: chunk shape {arr.chunks} differs from {shape}; tiles must be of equal shape')
        geometry.append((tuple(arr.shape[:2]), tuple(arr.chunks[:2])))
        for idx in arr.chunk_indices():
            if keep is not None and not keep[idx[0], idx[1]]:
                continue
            data = arr[arr.chunk_slices(idx)]
            hw.append(data.shape[:2])
            tiles.append(arr.pad_chunk(data))
    if not tiles:
        raise ValueError('no store given' if mask_group is None or not geometry else f'the masks {mask_group} leave no tile')
    return tiles, hw, geometry


class PatchSampler:
    """Patches of ``patch_size`` from ``pool``, uint8 ``[T, H, W, C]`` (``[T, H, W]``: one channel), 1 <= C <= 4.

    The argument names and defaults follow ``get_zarr_transform``: ``data_mode`` 'train' (random crop, padded where a tile
    is smaller than the patch) or 'test' (centre crop, tiles in order); ``add_noise`` adds N(0, noise_std^2) and clips to
    [0, 1]; ``normalize`` maps to [-1, 1]; ``rotation`` turns every patch by an angle uniform in [-degrees, degrees].
    ``tile_hw`` (``[T, 2]``) gives the valid rows and columns of each tile where the pool pads ragged tiles; padding is
    never sampled as image.  ``seed`` keys the noise.  ``force_torch=True`` computes the same contract with torch ops on
    the pool's device (the comparison of tools/bench_sampler.py; it is not a fallback: nothing selects it but this flag).
    ``elastic_deformation`` bends every patch after its rotation by ``elastic_deform`` with displacements drawn from
    N(0, ``elastic_sigma``^2) (``RandomElasticDeformationInput(sigma=10)``).

    Iterating yields ``steps_per_epoch`` batches ``(x, x)`` of ``batch_size`` patches.
    """

    def __init__(self, pool, patch_size: int, data_mode: str = 'train', add_noise: bool = False, noise_std: float = 0.001,
                 normalize: bool = False, rotation: bool = False, degrees: float = 30.0, seed: int = 0,
                 force_torch: bool = False, tile_hw=None, batch_size: int = 16, steps_per_epoch: Optional[int] = None,
                 elastic_deformation: bool = False, elastic_sigma: float = 10.0):
        pool = torch.as_tensor(pool)
        if pool.dim() == 3:
            pool = pool[..., None]
        if pool.dim() != 4 or pool.dtype != torch.uint8:
            raise ValueError(f'the pool is uint8 [T, H, W, C], got {pool.dtype} {tuple(pool.shape)}')
        if not 1 <= pool.shape[3] <= 4 or min(pool.shape[:3]) < 1:
            raise ValueError(f'the pool needs at least one tile and 1 to 4 channels, got {tuple(pool.shape)}')
        if 'train' in data_mode:
            self.data_mode = 'train'
        elif 'test' in data_mode:
            self.data_mode = 'test'
        else:
            raise ValueError(f"data_mode is 'train' or 'test', got {data_mode!r}")
        if int(patch_size) < 1:
            raise ValueError(f'patch_size {patch_size}')
        if not (noise_std >= 0.0 and math.isfinite(noise_std)):
            raise ValueError(f'noise_std {noise_std}')
        if not (elastic_sigma >= 0.0 and math.isfinite(elastic_sigma)):
            raise ValueError(f'elastic_sigma {elastic_sigma}')
        self.elastic_deformation, self.elastic_sigma = bool(elastic_deformation), float(elastic_sigma)
        self.pool = pool.contiguous()
        self.T, self.H, self.W, self.C = (int(v) for v in self.pool.shape)
        self.patch_size = int(patch_size)
        self.add_noise, self.noise_std = bool(add_noise), float(noise_std)
        self.normalize, self.rotation, self.degrees = bool(normalize), bool(rotation), float(degrees)
        self.seed = int(seed) & _M64
        self.force_torch = bool(force_torch)
        if tile_hw is None:
            self.tile_hw = torch.tensor([[self.H, self.W]], dtype=torch.int32).repeat(self.T, 1)
            self._ragged = False
        else:
            self.tile_hw = torch.as_tensor(tile_hw).to(torch.int32).cpu().reshape(self.T, 2).contiguous()
            if bool((self.tile_hw < 1).any()) or bool((self.tile_hw > torch.tensor([self.H, self.W])).any()):
                raise ValueError('tile_hw entries lie in [1, H] x [1, W]')
            self._ragged = True
        self.batch_size = int(batch_size)
        self.steps_per_epoch = int(steps_per_epoch) if steps_per_epoch is not None else -(-self.T // self.batch_size)
        self._batch = 0      # batches sampled so far: varies the noise seed
        self._next_tile = 0  # 'test': the next tile in order
        self._dev = None     # (pool, tile_hw) on the device, made on first use

    # ---- construction from slides ------------------------------------------------------------------------------------
    @classmethod
    def from_zarr(cls, stores: Sequence[str], data_group: str = '0/0', patch_size: int = 128,
                  mask_group: Optional[str] = None, **kwargs) -> 'PatchSampler':
        """A sampler over every chunk of the ``data_group`` array (Y, X, C uint8; or Y, X) of each store, read through
        ``ZarrArray.__getitem__``.  One tile per chunk: all stores share one chunk shape; the chunks on the lower and
        right edges of an image are padded to it (``ZarrArray.pad_chunk``) and keep their valid size.  ``mask_group``
        (the reference's ``--mask-group``, e.g. 'masks/0/0' of ``tissue.mask_zarr``): only the chunks that the store's
        mask touches enter the pool, in their order; ValueError when none is left."""
        tiles, hw, _ = _zarr_tiles(stores, data_group, mask_group)
        return cls(np.stack(tiles), patch_size, tile_hw=np.asarray(hw, dtype=np.int32), **kwargs)

    # ---- host: the random draws --------------------------------------------------------------------------------------
    def draw(self, n: int, generator: Optional[torch.Generator] = None):
        """``(tile, y0, x0, angle)`` of ``n`` patches with torchvision's policies; host code, no GPU needed.
        'train': the tile is uniform; per axis, the offset is uniform in [0, dim - ps] where the tile's valid dim >= ps and
        in [-(ps - dim), 0] where it is smaller (``RandomCrop(pad_if_needed)`` pads both sides by ps - dim).  'test': tiles in
        order (continuing where the last draw stopped) and the ``CenterCrop`` offset, int(round((dim - ps) / 2)) for
        dim >= ps, else -((ps - dim) // 2).  ``angle`` (degrees, float64) is uniform in [-degrees, degrees] with
        ``rotation``, else None.  The same generator state gives the same draw."""
        n, ps = int(n), self.patch_size
        if self.data_mode == 'train':
            r = torch.randint(0, 1 << 62, (3, n), generator=generator, dtype=torch.int64)
            tile = r[0] % self.T
            dims = self.tile_hw.to(torch.int64)[tile]  # [n, 2]
            span = (dims - ps).abs() + 1
            off = r[1:].t() % span + torch.clamp(dims - ps, max=0)
        else:
            tile = (self._next_tile + torch.arange(n, dtype=torch.int64)) % self.T
            self._next_tile = int((self._next_tile + n) % self.T)
            dims = self.tile_hw.to(torch.int64)[tile]
            # torchvision's center_crop: int(round((dim - ps) / 2.0)) (Python's round: half to even), padding (ps - dim) // 2
            off = torch.tensor([[int(round((d - ps) / 2.0)) if d >= ps else -((ps - d) // 2) for d in row]
                                for row in dims.tolist()], dtype=torch.int64).reshape(n, 2)
        angle = None
        if self.rotation:
            angle = self._draw_angle(n, generator)
        return tile.to(torch.int32), off[:, 0].to(torch.int32).contiguous(), off[:, 1].to(torch.int32).contiguous(), angle

    def _draw_angle(self, n: int, generator) -> torch.Tensor:
        """torchvision's RandomRotation: uniform in [-degrees, degrees]"""
        return (torch.rand(n, generator=generator, dtype=torch.float64) * 2.0 - 1.0) * self.degrees

    def draw_displacement(self, n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """The displacement grids of ``n`` patches, float64 ``[n, 2, 3, 3]``: ``np.random.randn(2, 3, 3) * sigma`` per
        patch.  Host code; ``sample`` calls it after ``draw``, and only with ``elastic_deformation``."""
        return torch.randn(int(n), 2, 3, 3, generator=generator, dtype=torch.float64) * self.elastic_sigma

    # ---- device: the batch -------------------------------------------------------------------------------------------
    def _device_pool(self):
        if self._dev is None:
            dev = self.pool.device if self.pool.is_cuda else _lib.require_gpu()
            self._dev = (self.pool.to(dev), self.tile_hw.to(dev) if self._ragged else None)
        return self._dev

    def _gather_args(self, tile, y0, x0, angle, noise_seed):
        """the arguments of ``gather`` as the entry points take them: int32 host vectors, ``n``, cos / sin ([2, n] float32
        or None), the noise seed and the noise's standard deviation"""
        tile, y0, x0 = (torch.as_tensor(v).to(torch.int32).cpu().reshape(-1).contiguous() for v in (tile, y0, x0))
        n = tile.numel()
        if y0.numel() != n or x0.numel() != n:
            raise ValueError('tile, y0 and x0 name one value per sample')
        cs = None
        if angle is not None:
            a = torch.deg2rad(torch.as_tensor(angle, dtype=torch.float64).cpu().reshape(-1))
            if a.numel() != n:
                raise ValueError('one angle per sample')
            cs = torch.stack([torch.cos(a), torch.sin(a)]).to(torch.float32)  # float64 on the host, rounded once
        seed = self.seed if noise_seed is None else int(noise_seed) & _M64
        std = self.noise_std if self.add_noise else 0.0
        return tile, y0, x0, n, cs, seed, std

    def gather(self, tile, y0, x0, angle=None, noise_seed: Optional[int] = None, sample_base: int = 0,
               displacement=None) -> torch.Tensor:
        """The ``[n, C, ps, ps]`` fp32 batch of the given draw on the device.  ``angle`` in degrees (None: no rotation).
        ``displacement`` (``[n, 2, 3, 3]``, None: no deformation) bends the rotated batch by ``elastic_deform``.
        ``noise_seed`` keys the noise of this batch (None: the sampler's ``seed``); it is used with ``add_noise`` only.
        ``sample_base`` is the index of the batch's first sample in the noise stream, so a batch can be gathered in
        parts.  A tile index outside the pool raises ValueError before anything is launched."""
        x = self._gather_plain(tile, y0, x0, angle, noise_seed, sample_base)
        return x if displacement is None else elastic_deform(x, displacement, force_torch=self.force_torch)

    def _gather_plain(self, tile, y0, x0, angle, noise_seed, sample_base) -> torch.Tensor:
        """``gather`` up to and including the rotation"""
        tile, y0, x0, n, cs, seed, std = self._gather_args(tile, y0, x0, angle, noise_seed)
        if self.force_torch:
            g = self.torch_normals(n, seed, int(sample_base)) if std != 0.0 else None
            return self._gather_torch(tile, y0, x0, cs, std, g)
        pool, tile_hw = self._device_pool()
        idx = torch.stack([tile, y0, x0]).to(pool.device)
        cs_dev = cs.to(pool.device) if cs is not None else None
        out = torch.empty((n, self.C, self.patch_size, self.patch_size), dtype=torch.float32, device=pool.device)
        with torch.cuda.device(pool.device):
            _lib.check(_lib.lib().cae_t_sample_patches(
                pool.data_ptr(), self.T, self.H, self.W, self.C, tile_hw.data_ptr() if tile_hw is not None else None,
                idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(), tile.data_ptr(),
                cs_dev[0].data_ptr() if cs is not None else None, cs_dev[1].data_ptr() if cs is not None else None,
                seed, int(sample_base) & 0xFFFFFFFF, std, int(self.normalize), n, self.patch_size, out.data_ptr(),
                _lib.stream_ptr()))
        return out

    def torch_normals(self, n: int, seed: int, sample_base: int = 0) -> torch.Tensor:
        """force_torch: the normals of a batch, ``[n, ps, ps, C]`` float32 on the pool's device, generated on the host."""
        ps = self.patch_size
        g = philox_normals(seed, (sample_base + np.arange(n, dtype=np.uint64))[:, None], np.arange(ps * ps, dtype=np.uint64))
        return torch.from_numpy(g[..., :self.C].astype(np.float32)).to(self.pool.device).reshape(n, ps, ps, self.C)

    def _gather_torch(self, tile, y0, x0, cs, std, g) -> torch.Tensor:
        """The contract as torch ops on the pool's device; the Philox normals ``g`` come from the host."""
        n, ps, dev = tile.numel(), self.patch_size, self.pool.device
        if n and (int(tile.min()) < 0 or int(tile.max()) >= self.T):
            raise ValueError(f'tile index outside the pool of {self.T} tiles')
        t = tile.to(dev).long()
        r = torch.arange(ps, device=dev)
        iy, ix = y0.to(dev).long()[:, None] + r, x0.to(dev).long()[:, None] + r  # [n, ps]
        hw = self.tile_hw.to(dev).long()[t]
        vy, vx = (iy >= 0) & (iy < hw[:, :1]), (ix >= 0) & (ix < hw[:, 1:])
        valid = (vy[:, :, None] & vx[:, None, :])[..., None]  # [n, ps, ps, 1]
        u8 = self.pool[t[:, None, None], iy.clamp(0, self.H - 1)[:, :, None], ix.clamp(0, self.W - 1)[:, None, :]]
        # the correctly rounded quotients as a table from the host (a device division by a scalar may multiply by 1 / 255)
        v = torch.arange(256, dtype=torch.float32).div(255).to(dev)[u8.long()]
        if std != 0.0:
            v = (v + std * g).clamp_(0, 1)
        v = torch.where(valid, v, torch.zeros((), dtype=v.dtype, device=dev))
        if self.normalize:
            v = (v - 0.5) / 0.5
        p = v.permute(0, 3, 1, 2).contiguous()
        if cs is None:
            return p
        c, s = cs[0].to(dev), cs[1].to(dev)
        z = torch.zeros_like(c)
        theta = torch.stack([torch.stack([c, -s, z], 1), torch.stack([s, c, z], 1)], 1)  # [n, 2, 3]
        grid = F.affine_grid(theta, list(p.shape), align_corners=False)
        return F.grid_sample(p, grid, mode='bilinear', padding_mode='zeros', align_corners=False)

    def batch_seed(self, batch: int) -> int:
        """The noise seed of the ``batch``-th sampled batch, derived from ``seed``."""
        return _splitmix64(_splitmix64(self.seed) ^ (int(batch) & _M64))

    def sample(self, n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``draw`` (then ``draw_displacement`` with ``elastic_deformation``) then ``gather``; every call takes the next
        per-batch noise seed."""
        tile, y0, x0, angle = self.draw(n, generator)
        displacement = self.draw_displacement(n, generator) if self.elastic_deformation else None
        x = self.gather(tile, y0, x0, angle, noise_seed=self.batch_seed(self._batch), displacement=displacement)
        self._batch += 1
        return x

    # ---- an epoch of batches, as the reference's data loader yields them -----------------------------------------------
    def __len__(self) -> int:
        return self.steps_per_epoch

    def __iter__(self):
        if self.data_mode == 'test':
            self._next_tile = 0
        for _ in range(self.steps_per_epoch):
            x = self.sample(self.batch_size)
            yield x, x


# ---- labelled patches: image and mask under one crop and one rotation ------------------------------------------------
# the poles and the gain of the quartic B-spline's inverse filter (contract: include/cae_hip.h, cae_t_sample_labeled_patches)
_SPLINE_POLES = (math.sqrt(664.0 - math.sqrt(438976.0)) + math.sqrt(304.0) - 19.0,
                 math.sqrt(664.0 + math.sqrt(438976.0)) - math.sqrt(304.0) - 19.0)
_SPLINE_GAIN = math.prod((1.0 - z) * (1.0 - 1.0 / z) for z in _SPLINE_POLES)
_LDS_PATCH = 128  # the entry point needs a workspace for rotated patches larger than this


def _spline_prefilter(c: np.ndarray, poles=_SPLINE_POLES, gain=_SPLINE_GAIN) -> np.ndarray:
    """force_torch: the interpolation coefficients along the last axis of float64 ``c``, every line at once (the quartic
    spline's poles and gain unless others are given)"""
    c = c * gain
    n = c.shape[-1]
    for z in poles:
        zn = z ** n
        mirrored = c[..., ::-1]
        acc = c[..., 0] + zn * mirrored[..., 0]
        if n > 1:
            acc = acc + ((c[..., 1:] + zn * mirrored[..., 1:]) * z ** np.arange(1, n)).sum(-1)
        c[..., 0] += z / (1.0 - zn * zn) * acc
        for i in range(1, n):
            c[..., i] += z * c[..., i - 1]
        c[..., n - 1] *= z / (z - 1.0)
        for i in range(n - 2, -1, -1):
            c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def _spline_weight(d: np.ndarray) -> np.ndarray:
    d = np.abs(d)
    return np.where(d < 0.5, d * d * (d * d / 4.0 - 5.0 / 8.0) + 115.0 / 192.0,
                    np.where(d < 1.5, d * (d * (d * (5.0 / 6.0 - d / 6.0) - 5.0 / 4.0) + 5.0 / 24.0) + 55.0 / 96.0,
                             np.where(d < 2.5, (d - 2.5) ** 4 / 24.0, 0.0)))


def _reflect(idx: np.ndarray, n: int) -> np.ndarray:
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


# ---- elastic deformation: a 3 x 3 displacement grid bent into a per-pixel field (contract: include/cae_hip.h) ------------
# the samples of the cubic B-spline at the three control points: displacement = M coefficient M^T
_ELASTIC_M = np.array([[2.0 / 3.0, 1.0 / 3.0, 0.0], [1.0 / 6.0, 2.0 / 3.0, 1.0 / 6.0], [0.0, 1.0 / 3.0, 2.0 / 3.0]])
_CUBIC_POLE, _CUBIC_GAIN = math.sqrt(3.0) - 2.0, 6.0


def elastic_coefficients(displacement: np.ndarray) -> np.ndarray:
    """``coef[k] = M^-1 d[k] M^-T`` of float64 displacement grids ``[n, 2, 3, 3]``, in float64"""
    inv = np.linalg.inv(_ELASTIC_M)
    return np.einsum('pa,nkab,qb->nkpq', inv, np.asarray(displacement, dtype=np.float64), inv)


def _cubic_weight(d: np.ndarray) -> np.ndarray:
    d = np.abs(d)
    return np.where(d < 1.0, 2.0 / 3.0 - d * d + d * d * d / 2.0, np.where(d < 2.0, (2.0 - d) ** 3 / 6.0, 0.0))


def _elastic_host(x: np.ndarray, t: Optional[np.ndarray], coef: np.ndarray):
    """The contract of ``cae_t_elastic_deform`` in float64 numpy: ``x`` ``[n, c, ps, ps]``, ``t`` ``[n, kt, ps, ps]`` or
    None, ``coef`` the float32 coefficients the kernel would get.  Returns float64 ``x'`` and ``t'`` (or None)."""
    n, ch, ps, _ = x.shape
    cf = _spline_prefilter(x.astype(np.float64), (_CUBIC_POLE,), _CUBIC_GAIN)                                  # rows
    cf = _spline_prefilter(cf.swapaxes(-1, -2).copy(), (_CUBIC_POLE,), _CUBIC_GAIN).swapaxes(-1, -2)         # columns
    u = 2.0 * np.arange(ps, dtype=np.float64) / (ps - 1) if ps > 1 else np.zeros(1)
    w = np.stack([_cubic_weight(u), _cubic_weight(u - 1.0) + _cubic_weight(u + 1.0) + _cubic_weight(u - 3.0),
                  _cubic_weight(u - 2.0)])
    with np.errstate(invalid='ignore', over='ignore'):
        field = np.einsum('ai,bj,nkab->nkij', w, w, coef.astype(np.float64))
    i, j = np.meshgrid(np.arange(ps, dtype=np.float64), np.arange(ps, dtype=np.float64), indexing='ij')
    x_out = np.zeros((n, ch, ps, ps))
    t_out = None if t is None else np.empty_like(t)
    for s in range(n):
        y = np.fmin(np.fmax(i + field[s, 0], -float(ps)), 2.0 * ps)  # fmax / fmin: a NaN becomes -ps
        xx = np.fmin(np.fmax(j + field[s, 1], -float(ps)), 2.0 * ps)
        if t is not None:
            t_out[s] = t[s][:, _reflect(np.floor(y + 0.5).astype(np.int64), ps), _reflect(np.floor(xx + 0.5).astype(np.int64), ps)]
        ys, xs = np.floor(y).astype(np.int64) - 1, np.floor(xx).astype(np.int64) - 1
        for a in range(4):
            wy, ry = _cubic_weight(y - (ys + a)), _reflect(ys + a, ps)
            for b in range(4):
                x_out[s] += wy * _cubic_weight(xx - (xs + b)) * cf[s][:, ry, _reflect(xs + b, ps)]
    return x_out, t_out


def elastic_workspace_bytes(n: int, c: int, ps: int) -> int:
    """the scratch ``cae_t_elastic_deform`` needs (its contract's formula)"""
    return int(n) * int(c) * int(ps) * int(ps) * 4 if ps > _LDS_PATCH else 0


def elastic_deform(x: torch.Tensor, displacement, t: Optional[torch.Tensor] = None, force_torch: bool = False):
    """The reference's elastic deformation of a batch on the device (``cae_t_elastic_deform``, contract in
    include/cae_hip.h): ``x`` fp32 ``[n, c, ps, ps]`` and optionally its masks ``t`` fp32 ``[n, kt, ps, ps]``, bent by the
    per-pixel field of the displacement grids ``displacement`` ``[n, 2, 3, 3]`` (float64 or float32, host or device; row
    displacements first).  The image goes through the interpolating cubic B-spline, the mask through its nearest
    neighbour, edges reflected.  Returns ``x'``, or ``(x', t')`` with ``t``.

    The spline coefficients of the grids are solved for in float64 on the host and rounded once.  There is no CPU
    fallback: without a HIP device the call raises RuntimeError.  ``force_torch=True`` evaluates the same contract in
    float64 on the host and uploads it to ``x``'s device: a comparison path that nothing but this flag selects."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or x.shape[2] != x.shape[3]:
        raise ValueError('expected an fp32 batch [n, c, ps, ps]')
    n, c, ps, _ = (int(v) for v in x.shape)
    if not 1 <= c <= 4 or ps < 1:
        raise ValueError(f'1 to 4 channels of at least one pixel, got {tuple(x.shape)}')
    d = torch.as_tensor(displacement)
    if d.dtype not in (torch.float64, torch.float32) or tuple(d.shape) != (n, 2, 3, 3):
        raise ValueError(f'the displacement is float64 or float32 [{n}, 2, 3, 3], got {d.dtype} {tuple(d.shape)}')
    kt = 0
    if t is not None:
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype != torch.float32:
            raise ValueError('expected fp32 masks [n, kt, ps, ps]')
        kt = int(t.shape[1])
        if (int(t.shape[0]), int(t.shape[2]), int(t.shape[3])) != (n, ps, ps) or not 1 <= kt <= 4 or t.device != x.device:
            raise ValueError(f'the masks {tuple(t.shape)} on {t.device} do not match the batch {tuple(x.shape)} on {x.device}')
    coef = elastic_coefficients(d.detach().cpu().to(torch.float64).numpy()).astype(np.float32)
    if force_torch:
        xo, to = _elastic_host(x.detach().cpu().numpy(), None if t is None else t.detach().cpu().numpy(), coef)
        xo = torch.from_numpy(xo.astype(np.float32)).to(x.device)
        return xo if t is None else (xo, torch.from_numpy(to).to(x.device))
    _lib.require_gpu()
    if not x.is_cuda:
        raise ValueError('expected the batch on the device')
    x = x.contiguous()
    t = t.contiguous() if t is not None else None
    coef_dev = torch.from_numpy(coef).to(x.device)
    x_out = torch.empty((n, c, ps, ps), dtype=torch.float32, device=x.device)
    t_out = torch.empty((n, kt, ps, ps), dtype=torch.float32, device=x.device) if t is not None else None
    ws_bytes = elastic_workspace_bytes(n, c, ps)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().cae_t_elastic_deform(
            x.data_ptr(), t.data_ptr() if t is not None else None, coef_dev.data_ptr(), n, c, kt, ps,
            ws.data_ptr() if ws is not None else None, ws_bytes, x_out.data_ptr(),
            t_out.data_ptr() if t is not None else None, _lib.stream_ptr()))
    return x_out if t is None else (x_out, t_out)


class WeightsDistances:
    """The reference's ``WeightsDistances`` (_augs.py:102-136) for a batch on the device: the U-Net border weight
    ``class_weights[t] + w_0 exp(-(d1 + d2)^2 / (2 sigma^2))``, d1 and d2 the distances to the nearest and second-nearest
    object of the plane (one object: ``exp(-d1^2 / (2 sigma^2))``; none: the class weight alone).

    Called on label planes ``t`` ``[n, 1, h, w]`` (fp32 or int64, integer values) on the device, returns fp32
    ``[n, 2, h, w]``: the weights, then the labels -- what ``SegLoss('WeightedBCELoss')`` takes.  The steps are
    ``segmenters.components(t != 0)``, ``segmenters.object_distances`` and ``cae_seg_weight_map`` (contract in
    include/cae_hip.h), then one read of the kernel's flag: a label outside ``class_weights`` raises IndexError, as
    ``numpy.take`` does.  ``force_torch=True`` runs the reference's own procedure on the host (``scipy.ndimage.label``
    and one ``distance_transform_edt`` per object) and uploads the result: a comparison path that nothing but this flag
    selects.
    """

    def __init__(self, class_weights, sigma=5, w_0=10, force_torch: bool = False):
        cw = np.asarray(class_weights, dtype=np.float32).reshape(-1)
        if cw.size < 1:
            raise ValueError('class_weights is empty')
        sigma_2 = float(np.float32(2 * float(sigma) ** 2))
        if not (math.isfinite(sigma_2) and sigma_2 > 0.0):
            raise ValueError(f'sigma {sigma}')
        self.class_weights = class_weights
        self.sigma_2 = 2 * sigma ** 2
        self.w_0 = w_0
        self.force_torch = bool(force_torch)
        self._cw, self._sigma_2 = cw, sigma_2
        self._cw_dev = None

    @staticmethod
    def _planes(t):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype not in (torch.float32, torch.int64):
            raise ValueError('expected label planes [n, 1, h, w], fp32 or int64')
        if t.shape[1] != 1:
            raise ValueError(f'the weight map is built for one target channel, got {t.shape[1]}')
        return t.to(torch.float32).contiguous()

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        return self.apply(t, check=True)

    @torch.no_grad()
    def apply(self, t: torch.Tensor, check: bool = True) -> torch.Tensor:
        """``__call__``; with ``check=False`` the flag is not read back (a caller that has checked its labels against
        the table before: the call then stays asynchronous)."""
        t = self._planes(t)
        if self.force_torch:
            return self._host(t)
        from . import segmenters
        _lib.require_gpu()
        if not t.is_cuda:
            raise ValueError('expected label planes on the device')
        n, _, h, w = t.shape
        dev = t.device
        with torch.cuda.device(dev):
            labels, count = segmenters.components((t[:, 0] != 0).to(torch.uint8))
            d2 = segmenters.object_distances(labels)
            if self._cw_dev is None or self._cw_dev.device != dev:
                self._cw_dev = torch.from_numpy(self._cw).to(dev)
            out = torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            if n:
                _lib.check(_lib.lib().cae_seg_weight_map(
                    t.data_ptr(), d2.data_ptr(), count.data_ptr(), self._cw_dev.data_ptr(), self._cw.size, self._sigma_2,
                    float(self.w_0), n, h * w, out.data_ptr(), flag.data_ptr(), _lib.stream_ptr()))
            if check and n and int(flag.item()):
                raise IndexError(f'a label lies outside the {self._cw.size} class weights')
        return out

    def _host(self, t: torch.Tensor) -> torch.Tensor:
        """the reference's ``__call__`` per plane, in numpy on the host"""
        from scipy.ndimage import distance_transform_edt, label
        planes = t.cpu().numpy()
        out = []
        for target in planes:  # [1, h, w]
            w_x = np.take(self._cw, target.astype(np.int32)).astype(np.float32)
            if target.sum() > 0:
                target_labels, num_objects = label(target[0], structure=np.ones((3, 3)))
                dist = []
                for obj in range(1, num_objects + 1):
                    remaining = np.ones_like(target[0])
                    remaining[target_labels == obj] = 0
                    dist.append(distance_transform_edt(remaining).astype(np.float32))
                dist = np.sort(np.stack(dist), axis=0)
                s = dist[0] + dist[1] if num_objects > 1 else dist[0]
                w_x = w_x + np.float32(self.w_0) * np.exp(-s ** 2 / np.float32(self._sigma_2))
            out.append(np.concatenate((w_x.astype(np.float32), target), axis=0))
        if not out:
            return torch.empty((0, 2) + tuple(t.shape[2:]), dtype=torch.float32, device=t.device)
        return torch.from_numpy(np.stack(out)).to(t.device)


class LabeledPatchSampler(PatchSampler):
    """Pairs of an image patch and its pixel labels: ``PatchSampler`` over ``pool`` plus ``labels``, uint8 ``[T, H, W, K]``
    (``[T, H, W]``: one channel), 1 <= K <= 4, of the pool's ``T, H, W``.  Image and mask share tile, crop window, ragged
    extent (``tile_hw``) and angle; the kernel call is ``cae_t_sample_labeled_patches`` (contract in include/cae_hip.h).

    Stands where ``get_zarr_transform`` with ``label_density == 2`` stands.  What differs from the unlabelled sampler is
    the reference's own difference: ``rotation`` turns the pair by an angle uniform in [0, degrees) (not symmetric;
    ``RandomRotationInputTarget``), the image through the exactly interpolating quartic B-spline and the mask through its
    nearest neighbour, both with reflected edges.  ``map_labels`` sums the K label channels into one (``MapLabels``);
    ``target_data_type`` is ``torch.float32`` or ``torch.int64`` (``ConvertTensorDtype``: a cast of the exact integer
    values).  ``force_torch=True`` computes the same contract in float64 on the host and uploads it: a comparison path
    that nothing but this flag selects.

    Iterating yields ``steps_per_epoch`` batches ``(x, t)``: ``x`` fp32 ``[n, C, ps, ps]`` and ``t`` ``[n, Kt, ps, ps]``
    (``Kt`` = 1 with ``map_labels``, else K), what ``seg_train.train_step`` and ``SegLoss('BCELoss')`` take; an int64 ``t``
    with ``Kt`` = 1 is yielded as ``[n, ps, ps]``, the class map ``SegLoss('CELoss')`` takes.

    ``class_weights``, ``weights_map_sigma`` and ``weights_map_w`` (all three, as in ``get_zarr_transform``, or none) add
    the reference's border weight map: ``t`` becomes fp32 ``[n, 2, ps, ps]``, ``WeightsDistances(class_weights,
    weights_map_sigma, weights_map_w)`` of the labels and then the labels, what ``SegLoss('WeightedBCELoss')`` takes.  It
    needs ``Kt`` = 1.  The map is computed on the final target, after crop and rotation, so the weights belong to the
    labels the loss sees (objects cut by the crop window count as the pieces that are left); the order of the reference's
    own pipeline lies in ``zarrdataset`` and is not pinned here.  The pool's largest label value (with ``map_labels`` the
    largest channel sum) is checked against ``class_weights`` once at construction -- IndexError -- so no batch reads the
    kernel's flag back.

    ``elastic_deformation`` bends image and labels after the pair's rotation by one field per sample
    (``RandomElasticDeformationInputTarget(sigma=10)``; ``elastic_deform``): the weight map is then taken on the deformed
    labels, and the cast to ``target_data_type`` comes last.
    """

    def __init__(self, pool, labels, patch_size: int, data_mode: str = 'train', add_noise: bool = False,
                 noise_std: float = 0.001, normalize: bool = False, rotation: bool = False, degrees: float = 30.0,
                 seed: int = 0, force_torch: bool = False, tile_hw=None, batch_size: int = 16,
                 steps_per_epoch: Optional[int] = None, map_labels: bool = False, target_data_type=torch.float32,
                 class_weights=None, weights_map_sigma=None, weights_map_w=None, elastic_deformation: bool = False,
                 elastic_sigma: float = 10.0):
        if target_data_type not in (torch.float32, torch.int64):
            raise ValueError('Convertion to data type {} not supported'.format(target_data_type))
        super().__init__(pool, patch_size, data_mode=data_mode, add_noise=add_noise, noise_std=noise_std, normalize=normalize,
                         rotation=rotation, degrees=degrees, seed=seed, force_torch=force_torch, tile_hw=tile_hw,
                         batch_size=batch_size, steps_per_epoch=steps_per_epoch, elastic_deformation=elastic_deformation,
                         elastic_sigma=elastic_sigma)
        labels = torch.as_tensor(labels)
        if labels.dim() == 3:
            labels = labels[..., None]
        if labels.dim() != 4 or labels.dtype != torch.uint8:
            raise ValueError(f'the labels are uint8 [T, H, W, K], got {labels.dtype} {tuple(labels.shape)}')
        if tuple(labels.shape[:3]) != (self.T, self.H, self.W):
            raise ValueError(f'the labels {tuple(labels.shape[:3])} do not match the pool {(self.T, self.H, self.W)}')
        if not 1 <= labels.shape[3] <= 4:
            raise ValueError(f'1 to 4 label channels, got {labels.shape[3]}')
        self.labels = labels.to(self.pool.device).contiguous()
        self.K = int(labels.shape[3])
        self.map_labels = bool(map_labels)
        self.Kt = 1 if self.map_labels else self.K
        self.target_data_type = target_data_type
        self._labels_dev = None
        self.weights = None
        given = [v is not None for v in (class_weights, weights_map_sigma, weights_map_w)]
        if any(given):
            if not all(given):
                raise ValueError('class_weights, weights_map_sigma and weights_map_w are given together or not at all')
            if self.Kt != 1:
                raise ValueError(f'the weight map needs one target channel, got {self.Kt} (map_labels sums them into one)')
            self.weights = WeightsDistances(class_weights, sigma=weights_map_sigma, w_0=weights_map_w,
                                            force_torch=self.force_torch)
            top = int(self.labels.sum(dim=3, dtype=torch.int64).max()) if self.map_labels else int(self.labels.max())
            if top >= self.weights._cw.size:
                raise IndexError(f'the largest label value {top} lies outside the {self.weights._cw.size} class weights')

    @classmethod
    def from_zarr(cls, stores: Sequence[str], data_group: str = '0/0', labels_data_group: str = 'labels/0/0',
                  patch_size: int = 128, mask_group: Optional[str] = None, **kwargs) -> 'LabeledPatchSampler':
        """``PatchSampler.from_zarr`` for both arrays of each store: the image (Y, X, C) under ``data_group`` and the
        labels (Y, X, K; or Y, X) under ``labels_data_group``, both read through ``ZarrArray``.  The two arrays of a store
        must agree in Y / X shape and chunking (ValueError otherwise), so a chunk of one is the tile of the other; ragged
        edge tiles keep their valid size for both.  ``mask_group``: one selection of chunks for image and labels, as in
        ``PatchSampler.from_zarr``."""
        tiles, hw, geometry = _zarr_tiles(stores, data_group, mask_group)
        masks, mask_hw, mask_geometry = _zarr_tiles(stores, labels_data_group, mask_group)
        for store, g, mg in zip([stores] if isinstance(stores, str) else stores, geometry, mask_geometry):
            if g != mg:
                raise ValueError(f'{store}: image {data_group} has (Y, X) shape and chunks {g}, labels {labels_data_group} '
                                 f'have {mg}; the two must agree')
        assert hw == mask_hw
        return cls(np.stack(tiles), np.stack(masks), patch_size, tile_hw=np.asarray(hw, dtype=np.int32), **kwargs)

    def _draw_angle(self, n: int, generator) -> torch.Tensor:
        """RandomRotationInputTarget: ``np.random.rand() * degrees``, uniform in [0, degrees)"""
        return torch.rand(n, generator=generator, dtype=torch.float64) * self.degrees

    def workspace_bytes(self, n: int, rotated: bool) -> int:
        """the scratch ``cae_t_sample_labeled_patches`` needs for ``n`` patches (its contract's formula)"""
        ps = self.patch_size
        return int(n) * self.C * ps * ps * 4 if rotated and ps > _LDS_PATCH else 0

    def gather(self, tile, y0, x0, angle=None, noise_seed: Optional[int] = None, sample_base: int = 0, displacement=None):
        """``(x, t)`` of the given draw on the device: ``x`` fp32 ``[n, C, ps, ps]``, ``t`` ``[n, Kt, ps, ps]`` in
        ``target_data_type``.  The arguments are those of ``PatchSampler.gather``; one ``angle`` turns image and mask, and
        one ``displacement`` grid per sample bends both."""
        x, t = self._gather_pair(tile, y0, x0, angle, noise_seed, sample_base)
        if displacement is not None:
            x, t = elastic_deform(x, displacement, t, force_torch=self.force_torch)
        return x, self._target(t)

    def _gather_pair(self, tile, y0, x0, angle, noise_seed, sample_base):
        """``gather`` up to and including the rotation: ``x`` and the fp32 labels"""
        tile, y0, x0, n, cs, seed, std = self._gather_args(tile, y0, x0, angle, noise_seed)
        ps = self.patch_size
        if self.force_torch:
            g = self.torch_normals(n, seed, int(sample_base)) if std != 0.0 else None
            return self._gather_host(tile, y0, x0, cs, std, g)
        pool, tile_hw = self._device_pool()
        if self._labels_dev is None:
            self._labels_dev = self.labels.to(pool.device)
        idx = torch.stack([tile, y0, x0]).to(pool.device)
        cs_dev = cs.to(pool.device) if cs is not None else None
        x = torch.empty((n, self.C, ps, ps), dtype=torch.float32, device=pool.device)
        t = torch.empty((n, self.Kt, ps, ps), dtype=torch.float32, device=pool.device)
        ws_bytes = self.workspace_bytes(n, cs is not None)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pool.device) if ws_bytes else None
        with torch.cuda.device(pool.device):
            _lib.check(_lib.lib().cae_t_sample_labeled_patches(
                pool.data_ptr(), self._labels_dev.data_ptr(), self.T, self.H, self.W, self.C, self.K,
                tile_hw.data_ptr() if tile_hw is not None else None, idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(),
                tile.data_ptr(), cs_dev[0].data_ptr() if cs is not None else None,
                cs_dev[1].data_ptr() if cs is not None else None, seed, int(sample_base) & 0xFFFFFFFF, std,
                int(self.normalize), int(self.map_labels), n, ps, ws.data_ptr() if ws is not None else None, ws_bytes,
                x.data_ptr(), t.data_ptr(), _lib.stream_ptr()))
        return x, t

    def _target(self, t: torch.Tensor) -> torch.Tensor:
        """the fp32 labels ``[n, Kt, ps, ps]`` as the sampler hands them out: cast, or with their weight map in front"""
        if self.weights is None:
            return t.to(self.target_data_type)
        return self.weights.apply(t, check=False)  # the pool's labels were checked against the table at construction

    def _gather_host(self, tile, y0, x0, cs, std, g):
        """The contract in float64 numpy on the host, uploaded as float32 to the pool's device.  The patch ``p`` is
        ``PatchSampler``'s torch form; the label window is gathered the same way."""
        n, ps, dev = tile.numel(), self.patch_size, self.pool.device
        p = self._gather_torch(tile, y0, x0, None, std, g)  # [n, C, ps, ps] float32: p of the contract
        t_ = tile.to(dev).long()
        r = torch.arange(ps, device=dev)
        iy, ix = y0.to(dev).long()[:, None] + r, x0.to(dev).long()[:, None] + r
        hw = self.tile_hw.to(dev).long()[t_]
        vy, vx = (iy >= 0) & (iy < hw[:, :1]), (ix >= 0) & (ix < hw[:, 1:])
        m = self.labels[t_[:, None, None], iy.clamp(0, self.H - 1)[:, :, None], ix.clamp(0, self.W - 1)[:, None, :]]
        m = torch.where((vy[:, :, None] & vx[:, None, :])[..., None], m, torch.zeros((), dtype=m.dtype, device=dev))
        m = m.permute(0, 3, 1, 2).to(torch.float32)
        if self.map_labels:
            m = m.sum(dim=1, keepdim=True)
        if cs is None:
            return p, m.contiguous()
        coef = _spline_prefilter(p.cpu().numpy().astype(np.float64))                # rows
        coef = _spline_prefilter(coef.swapaxes(-1, -2).copy()).swapaxes(-1, -2)     # columns
        mask = m.cpu().numpy()
        c = (ps - 1) / 2.0
        i, j = np.meshgrid(np.arange(ps, dtype=np.float64), np.arange(ps, dtype=np.float64), indexing='ij')
        x_out, t_out = np.zeros((n, self.C, ps, ps)), np.empty((n, self.Kt, ps, ps), dtype=np.float32)
        for s in range(n):
            ca, sa = float(cs[0, s]), float(cs[1, s])
            y, x = ca * (i - c) + sa * (j - c) + c, -sa * (i - c) + ca * (j - c) + c
            ny, nx = np.floor(y + 0.5).astype(np.int64), np.floor(x + 0.5).astype(np.int64)
            t_out[s] = mask[s][:, _reflect(ny, ps), _reflect(nx, ps)]
            for a in range(5):
                wy, ry = _spline_weight(y - (ny - 2 + a)), _reflect(ny - 2 + a, ps)
                for b in range(5):
                    x_out[s] += wy * _spline_weight(x - (nx - 2 + b)) * coef[s][:, ry, _reflect(nx - 2 + b, ps)]
        return torch.from_numpy(x_out.astype(np.float32)).to(dev), torch.from_numpy(t_out).to(dev)

    def sample(self, n: int, generator: Optional[torch.Generator] = None):
        """``draw`` (then ``draw_displacement`` with ``elastic_deformation``) then ``gather`` -> ``(x, t)``; every call
        takes the next per-batch noise seed."""
        tile, y0, x0, angle = self.draw(n, generator)
        displacement = self.draw_displacement(n, generator) if self.elastic_deformation else None
        pair = self.gather(tile, y0, x0, angle, noise_seed=self.batch_seed(self._batch), displacement=displacement)
        self._batch += 1
        return pair

    def __iter__(self):
        if self.data_mode == 'test':
            self._next_tile = 0
        for _ in range(self.steps_per_epoch):
            x, t = self.sample(self.batch_size)
            yield x, (t[:, 0] if self.Kt == 1 and self.target_data_type == torch.int64 and self.weights is None else t)
