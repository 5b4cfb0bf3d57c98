"""Region reads of zarr arrays (ZarrArray.__getitem__ / read_region) and the ABI of the scaled synthesis: CPU tests.

A region read must equal numpy basic indexing of the source array, and it must read and decode only the chunks the key
touches, each once."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cnn_autoencoder_amd import zarrio


class CountingZlib(zarrio.Zlib):
    """Zlib that records every decode, keyed by the chunk's content tag (first byte pair = chunk number)."""

    def __init__(self, level=1):
        super().__init__(level)
        self.decoded = []

    def decode(self, buf, out=None):
        arr = super().decode(buf, out)
        self.decoded.append(bytes(buf))
        return arr


def _store(tmp_path, a, chunks, codec, name='a'):
    z = zarrio.ZarrArray.create(str(tmp_path), name, a.shape, chunks, a.dtype, codec=codec)
    z[:] = a
    return z


def _random_key(rng, shape):
    key = []
    for n in shape[:int(rng.integers(0, len(shape) + 1))]:
        if rng.random() < 0.25:
            key.append(int(rng.integers(-n, n)))
        else:
            lo, hi = (int(v) for v in rng.integers(-n - 2, n + 3, 2))
            key.append(slice(lo if rng.random() < 0.8 else None, hi if rng.random() < 0.8 else None))
    if rng.random() < 0.3:
        key.insert(int(rng.integers(0, len(key) + 1)), Ellipsis)
    return tuple(key)


@pytest.mark.parametrize('seed', range(8))
@pytest.mark.parametrize('codec', ['raw', 'zlib'])
def test_region_reads_equal_numpy_slicing(tmp_path, seed, codec):
    rng = np.random.default_rng(seed)
    nd = int(rng.integers(1, 4))
    shape = tuple(int(v) for v in rng.integers(1, 24, nd))
    chunks = tuple(int(v) for v in rng.integers(1, 9, nd))  # mostly do not divide the shape
    a = rng.integers(0, 60000, shape).astype([np.uint8, np.uint16, np.float32][seed % 3])
    z = _store(tmp_path, a, chunks, zarrio.Zlib(1) if codec == 'zlib' else None)
    z = zarrio.ZarrArray.open(str(tmp_path), 'a')
    n_checked = 0
    for _ in range(60):
        key = _random_key(rng, shape)
        try:
            want = a[key]
        except IndexError:  # an integer that landed on a shorter dimension behind the Ellipsis
            with pytest.raises(IndexError):
                z[key]
            continue
        got = z[key]
        assert got.dtype == a.dtype and got.shape == want.shape, (shape, chunks, key)
        assert np.array_equal(got, want), (shape, chunks, key)
        n_checked += 1
    assert n_checked >= 30


def test_region_edges_of_chunks(tmp_path):
    """keys that start and end inside, on and across chunk edges; single rows; integers; negative bounds; empty"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 255, (37, 29, 3)).astype(np.uint8)
    z = _store(tmp_path, a, (8, 10, 3), zarrio.Zlib(1))
    marks = [0, 1, 7, 8, 9, 15, 16, 17, 28, 29, 36, 37]
    for y0 in marks:
        for y1 in marks:
            for x0, x1 in ((0, 29), (3, 7), (10, 20), (9, 21), (10, 11), (28, 29), (20, 20), (25, 4)):
                key = (slice(y0, y1), slice(x0, x1))
                assert np.array_equal(z[key], a[key]), key
    for key in [5, -1, (8, 10), (-37, -29, -3), (slice(-5, None), slice(None, -20)), (slice(16, 17),), (..., 1),
                (3, ..., slice(1, 3)), (slice(40, 50),), (slice(-100, 100), slice(-100, 2)), (), Ellipsis,
                (np.int64(4), slice(None)), slice(None)]:
        want = a[key]
        got = z[key]
        assert got.shape == want.shape and np.array_equal(got, want), key


def test_only_touched_chunks_are_decoded_each_once(tmp_path):
    a = np.zeros((40, 50), dtype=np.uint16)
    chunks = (8, 10)
    for i in range(5):
        for j in range(5):
            a[i * 8:(i + 1) * 8, j * 10:(j + 1) * 10] = 100 * i + j + 1  # chunk bytes differ -> identify the chunk
    codec = CountingZlib(1)
    z = _store(tmp_path, a, chunks, codec)
    stored = {z.read_chunk_bytes((i, j)): (i, j) for i in range(5) for j in range(5)}
    assert len(stored) == 25
    for key, want in [((slice(9, 23), slice(10, 20)), {(1, 1), (2, 1)}),
                      ((slice(8, 16), slice(0, 50)), {(1, j) for j in range(5)}),
                      ((17, slice(19, 21)), {(2, 1), (2, 2)}),
                      ((slice(7, 9), slice(9, 11)), {(0, 0), (0, 1), (1, 0), (1, 1)}),
                      ((slice(39, 40), slice(49, 50)), {(4, 4)}),
                      ((slice(3, 3), slice(0, 50)), set()),
                      (Ellipsis, {(i, j) for i in range(5) for j in range(5)})]:
        codec.decoded.clear()
        assert np.array_equal(z[key], a[key])
        seen = [stored[b] for b in codec.decoded]
        assert len(seen) == len(set(seen)), ('a chunk was decoded twice', key, seen)
        assert set(seen) == want, (key, seen)
        # read_region at scale 0 on a non-'cae' array is the same read
        codec.decoded.clear()
        assert np.array_equal(z.read_region(key), a[key])
        assert sorted(stored[b] for b in codec.decoded) == sorted(want)


def test_region_survives_deleted_untouched_chunks(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.integers(1, 255, (30, 30, 3)).astype(np.uint8)
    z = _store(tmp_path, a, (8, 8, 3), zarrio.Zlib(1))
    key = (slice(9, 15), slice(17, 30))
    keep = {(1, 2, 0), (1, 3, 0)}
    for idx in z.chunk_indices():
        if idx not in keep:
            os.remove(z.chunk_path(idx))
    z = zarrio.ZarrArray.open(str(tmp_path), 'a')
    assert np.array_equal(z[key], a[key])
    # a missing chunk under the key reads as fill_value
    got = z[slice(0, 15), slice(17, 30)]
    assert np.array_equal(got[9:], a[9:15, 17:30]) and not got[:8].any()


def test_bad_keys_raise(tmp_path):
    a = np.arange(6 * 7, dtype=np.uint8).reshape(6, 7)
    z = _store(tmp_path, a, (4, 4), None)
    with pytest.raises(IndexError, match='too many indices for array; expected 2, got 3'):
        z[0, 0, 0]
    with pytest.raises(IndexError, match='index out of bounds for dimension with length 6'):
        z[6]
    with pytest.raises(IndexError, match='index out of bounds for dimension with length 7'):
        z[0, -8]
    with pytest.raises(IndexError, match='single ellipsis'):
        z[..., ...]
    with pytest.raises(NotImplementedError, match='step 1'):
        z[::2]
    with pytest.raises(NotImplementedError, match='step 1'):
        z[:, ::-1]
    for key in ([0, 1], np.array([0, 1]), None, (0, None), 1.5, 'a', True, np.zeros(6, bool)):
        with pytest.raises(IndexError, match='unsupported selection item for basic indexing'):
            z[key]
    # region writes stay whole-array
    with pytest.raises(NotImplementedError):
        z[0:2] = a[0:2]
    z[:] = a
    assert np.array_equal(z[:], a)


def test_scale_needs_a_cae_array(tmp_path):
    a = np.zeros((16, 16, 3), dtype=np.uint8)
    for name, codec in (('raw', None), ('zl', zarrio.Zlib(1))):
        z = _store(tmp_path, a, (8, 8, 3), codec, name=name)
        with pytest.raises(ValueError, match="scale > 0 needs an array whose codec is 'cae'"):
            z.read_region((slice(0, 8), slice(0, 8)), scale=1)
        with pytest.raises(ValueError, match="scale > 0 needs an array whose codec is 'cae'"):
            zarrio.decompress_image(str(tmp_path), name, roi=(0, 8, 0, 8), scale=2)
        with pytest.raises(ValueError, match='scale'):
            z.read_region(Ellipsis, scale=-1)
        assert np.array_equal(zarrio.decompress_image(str(tmp_path), name, roi=(3, 11, 2, 9)), a[3:11, 2:9])


def test_abi_declares_and_binds_the_scaled_synthesis(built_lib):
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'cae_hip.h')).read()
    declared = set(re.findall(r'\b(cae_[a-z0-9_]+)\s*\(', hdr))
    L = ctypes.CDLL(cae.LIB_PATH)
    for name in ('cae_synthesis_scale', 'cae_synthesis_symbols_scale'):
        assert name in declared, f'{name} is not declared in include/cae_hip.h'
        assert name in _lib.SYMBOLS, f'{name} is not bound in _lib.py'
        assert hasattr(L, name), f'{name} is not exported by the library'
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == 9  # (m, in, n, lh, lw, scale, out, fmt, stream)
    assert declared == set(_lib.SYMBOLS)
