"""The device rANS coder (cae_rans_encode_device / cae_rans_decode_device, csrc/cae_rans_device.hip) against the host
coder and the oracle: identical bytes, identical symbols, the host's error conditions, and the coder='device' paths of
the Python surface (EntropyBottleneck, ConvolutionalAutoencoder, SlideCoder, zarrio)."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLD
from oracle import c_oracle as C


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    return cae


class _Tables:
    """A handle with explicit integer tables, coded on the host (cae_rans_*_batch) and on the device."""

    def __init__(self, cdf, lens, off):
        from cnn_autoencoder_amd import _lib
        self._lib = _lib
        self.set(cdf, lens, off, _lib.Handle(1, 1, np.asarray(cdf).shape[0], 1, 3))

    def set(self, cdf, lens, off, handle=None):
        self.cdf = np.ascontiguousarray(cdf, dtype=np.int32)
        self.lens = np.ascontiguousarray(lens, dtype=np.int32)
        self.off = np.ascontiguousarray(off, dtype=np.int32)
        self.C = self.cdf.shape[0]
        self.h = handle or self.h
        med = np.zeros(self.C, dtype=np.float32)
        self._lib.check(self._lib.lib().cae_model_set_entropy(self.h.ptr, self.C, self.cdf.shape[1], self.cdf.ctypes.data,
                                                              self.lens.ctypes.data, self.off.ctypes.data, med.ctypes.data))

    def encode_host(self, sym):
        sym = np.ascontiguousarray(sym, dtype=np.int32)
        n, hw = sym.shape[0], sym.shape[2]
        bufs = (ctypes.c_void_p * n)()
        lens = (ctypes.c_size_t * n)()
        self._lib.check(self._lib.lib().cae_rans_encode_batch(self.h.ptr, sym.ctypes.data, n, hw, bufs, lens, 0))
        out = [ctypes.string_at(bufs[i], lens[i]) for i in range(n)]
        for i in range(n):
            self._lib.lib().cae_free(bufs[i])
        return out

    def decode_host(self, strings, hw):
        n = len(strings)
        bufs = (ctypes.c_char_p * n)(*strings)
        lens = (ctypes.c_size_t * n)(*[len(s) for s in strings])
        sym = np.empty((n, self.C, hw), dtype=np.int32)
        self._lib.check(self._lib.lib().cae_rans_decode_batch(self.h.ptr, bufs, lens, n, hw, sym.ctypes.data, 0))
        return sym

    def encode_device(self, sym):
        from cnn_autoencoder_amd.entropy import rans_encode_device
        packed, offsets = rans_encode_device(self.h, torch.from_numpy(np.ascontiguousarray(sym, dtype=np.int32)).cuda())
        host = packed[:offsets[-1]].cpu().numpy().tobytes()
        return [host[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]

    def decode_device(self, strings, hw):
        from cnn_autoencoder_amd.entropy import rans_decode_device
        return rans_decode_device(self.h, self.C, strings, hw).cpu().numpy()

    def oracle_encode(self, sym_one):
        idx = np.repeat(np.arange(self.C), sym_one.shape[1]).astype(np.int32)
        return C.rans_encode_with_indexes(sym_one.reshape(-1), idx, self.cdf, self.lens, self.off)


def _random_tables(rng, channels, max_len):
    """as test_oracle._random_tables: rows of different lengths"""
    from test_oracle import _random_tables as rt
    return rt(rng, channels, max_len)


# ---- without a device: argument checks ---------------------------------------------------------------------------------
def test_device_abi_rejects_bad_arguments_without_a_device(cae):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    t = _Tables([[0, 32768, 65536]], [3], [0])
    fresh = _lib.Handle(1, 1, 1, 1, 3)  # no entropy tables
    fake = 1 << 20  # 16-byte aligned and never dereferenced: every call below fails its argument check first
    size = ctypes.c_size_t()
    assert L.cae_rans_encode_workspace(t.h.ptr, 4, 16, ctypes.byref(size)) == 0 and size.value >= 4 * (16 + 2) * 4
    for args in ((None, 4, 16), (t.h.ptr, 0, 16), (t.h.ptr, 4, 0), (fresh.ptr, 4, 16)):
        assert L.cae_rans_encode_workspace(args[0], args[1], args[2], ctypes.byref(size)) == -1
    assert L.cae_rans_encode_workspace(t.h.ptr, 4, 16, None) == -1
    # one grid row per stream: 65535 streams at the most
    assert L.cae_rans_encode_workspace(t.h.ptr, 65535, 16, ctypes.byref(size)) == 0
    assert L.cae_rans_encode_workspace(t.h.ptr, 65536, 16, ctypes.byref(size)) == -1
    assert b'65535' in L.cae_last_error()

    def enc(h=t.h.ptr, sym=fake, n=4, hw=16, out=fake, offs=fake, status=fake, ws=fake, ws_bytes=1 << 20):
        return L.cae_rans_encode_device(h, sym, n, hw, out, 1 << 20, offs, status, ws, ws_bytes, None)

    for kw in (dict(h=None), dict(sym=None), dict(out=None), dict(offs=None), dict(status=None), dict(ws=None),
               dict(n=0), dict(n=-3), dict(hw=0), dict(hw=-1), dict(h=fresh.ptr), dict(ws_bytes=64), dict(out=fake + 4)):
        assert enc(**kw) == -1, kw
        assert L.cae_last_error()

    def dec(h=t.h.ptr, buf=fake, offs=fake, n=4, hw=16, sym=fake, status=fake):
        return L.cae_rans_decode_device(h, buf, 64, offs, n, hw, sym, status, None)

    for kw in (dict(h=None), dict(buf=None), dict(offs=None), dict(sym=None), dict(status=None), dict(n=0), dict(hw=0),
               dict(h=fresh.ptr)):
        assert dec(**kw) == -1, kw


def test_unknown_coder_is_rejected(cae):
    eb = cae.EntropyBottleneck(4)
    eb.update()
    with pytest.raises(ValueError, match='coder'):
        eb.compress(torch.rand(1, 4, 2, 2), coder='gpu')
    with pytest.raises(ValueError, match='coder'):
        eb.decompress([b'\x00' * 8], (2, 2), coder='cpu')


# ---- on the device ----------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@gpu
def test_device_known_answers(cae):
    kat = json.load(open(os.path.join(GOLD, 'rans_kat.json')))['rans']
    for k in kat:
        t = _Tables(k['cdf'], k['cdf_length'], k['offset'])
        sym = np.asarray(k['symbols'], dtype=np.int32).reshape(1, len(k['cdf']), k['hw'])
        assert t.encode_device(sym)[0].hex() == k['bytes_hex'], k['name']
        assert np.array_equal(t.decode_device([bytes.fromhex(k['bytes_hex'])], k['hw']), sym), k['name']


@gpu
@pytest.mark.parametrize('seed,spread', [(0, 2), (1, 6), (2, 40), (3, 5000), (4, 2 ** 20), (5, 2 ** 26)])
def test_device_coder_bit_exact_vs_oracle(cae, seed, spread):
    rng = np.random.default_rng(200 + seed)
    channels, hw, n = int(rng.integers(1, 9)), int(rng.integers(1, 130)), 7
    t = _Tables(*_random_tables(rng, channels, 40))
    sym = rng.integers(-spread, spread + 1, (n, channels, hw)).astype(np.int32)
    out = t.encode_device(sym)
    assert out == [t.oracle_encode(sym[i]) for i in range(n)]
    assert out == t.encode_host(sym)
    assert np.array_equal(t.decode_device(out, hw), sym)


@gpu
def test_device_reciprocal_division_is_exact_for_every_frequency(cae):
    """every frequency 1..65535 on the device (two-bin rows [0, f, 65536]), against the oracle's plain division"""
    freqs = np.arange(1, 65536, dtype=np.int64)
    rng = np.random.default_rng(7)
    for block in np.array_split(freqs, 16):
        cdf = np.zeros((len(block), 3), dtype=np.int32)
        cdf[:, 1] = block
        cdf[:, 2] = 65536
        t = _Tables(cdf, np.full(len(block), 3, dtype=np.int32), np.zeros(len(block), dtype=np.int32))
        sym = rng.integers(0, 2, (2, len(block), 24)).astype(np.int32)  # value 1 = escape bin (freq 65536-f)
        out = t.encode_device(sym)
        assert out == [t.oracle_encode(sym[i]) for i in range(2)]
        assert np.array_equal(t.decode_device(out, 24), sym)


@gpu
def test_cross_decoding(cae):
    rng = np.random.default_rng(11)
    t = _Tables(*_random_tables(rng, 12, 30))
    sym = rng.integers(-40, 41, (9, 12, 77)).astype(np.int32)
    on_device, on_host = t.encode_device(sym), t.encode_host(sym)
    assert np.array_equal(t.decode_host(on_device, 77), sym)
    assert np.array_equal(t.decode_device(on_host, 77), sym)


@gpu
@pytest.mark.parametrize('n,hw,channels', [(1, 1, 1), (63, 65, 7), (64, 1, 192), (65, 130, 3), (130, 63, 40),
                                           (2, 200, 192), (64, 64, 1)])
def test_ragged_shapes(cae, n, hw, channels):
    """streams around the 64-lane workgroup, hw around the 64-symbol staging chunk, 1..192 channels, rows of
    different lengths"""
    rng = np.random.default_rng(n * 1000 + hw + channels)
    t = _Tables(*_random_tables(rng, channels, 60))
    sym = rng.integers(-30, 31, (n, channels, hw)).astype(np.int32)
    out = t.encode_device(sym)
    assert out == t.encode_host(sym)
    assert np.array_equal(t.decode_device(out, hw), sym)


@gpu
def test_table_change_is_seen_by_the_next_call(cae):
    rng = np.random.default_rng(5)
    t = _Tables(*_random_tables(rng, 6, 20))
    sym = rng.integers(-10, 11, (3, 6, 50)).astype(np.int32)
    first = t.encode_device(sym)
    t.set(*_random_tables(rng, 6, 33))
    second = t.encode_device(sym)
    assert second == t.encode_host(sym) and second != first


@gpu
def test_bad_input_raises_and_does_not_hang(cae):
    rng = np.random.default_rng(0)
    t = _Tables(*_random_tables(rng, 3, 10))
    with pytest.raises(ValueError, match='codable range'):
        t.encode_device(np.asarray([[[2 ** 29]] * 3], dtype=np.int32))
    sym = rng.integers(-3, 4, (1, 3, 300)).astype(np.int32)
    s = t.encode_device(sym)[0]
    for bad in (s[:4], s[:len(s) // 2], b'\x00' * len(s), b'\x00' * 8, s[:-3]):
        with pytest.raises(cae.CaeError, match='bitstream'):
            t.decode_device([bad], 300)
        with pytest.raises(cae.CaeError, match='bitstream'):
            t.decode_host([bad], 300)
    # bit flips: the device reaches the host's verdict (an error, or the same symbols)
    for bit in (0, 37, 8 * len(s) // 2, 8 * len(s) - 1):
        flipped = bytearray(s)
        flipped[bit // 8] ^= 1 << (bit % 8)
        flipped = bytes(flipped)
        try:
            ref = t.decode_host([flipped], 300)
        except cae.CaeError:
            with pytest.raises(cae.CaeError, match='bitstream'):
                t.decode_device([flipped], 300)
        else:
            assert np.array_equal(t.decode_device([flipped], 300), ref)
    # a damaged stream among good ones: reported, the batch raises
    with pytest.raises(cae.CaeError, match='bitstream'):
        t.decode_device([s, s[:6], s], 300)


def _canonical_codec(cae):
    from cnn_autoencoder_amd import synth
    state = synth.synthetic_state(synth.CANONICAL, seed=0)
    codec = cae.ConvolutionalAutoencoder(checkpoint=state)
    eb = codec._model['fact_ent'].module
    eb.fit_quantiles()
    eb.update(force=True)
    return codec, eb


@gpu
def test_whole_model_1024(cae):
    from cnn_autoencoder_amd import synth
    codec, eb = _canonical_codec(cae)
    tiles = np.stack([synth.histo_tile(1024, 0), synth.histo_tile(1024, 1), synth.uniform_tiles(1, 1024)[0]])
    host = codec.encode_batch(tiles)
    dev = codec.encode_batch(tiles, coder='device')
    assert dev == host
    assert np.array_equal(codec.decode_batch(dev, coder='device'), codec.decode_batch(host))
    # the entropy bottleneck's own surface
    y = codec._model['encoder'].module.forward_u8(torch.from_numpy(tiles).cuda())
    strings = eb.compress(y, coder='device')
    assert strings == eb.compress(y) == [b[16:] for b in host]
    assert torch.equal(eb.decompress(strings, (64, 64), coder='device'), eb.decompress(strings, (64, 64)))


@gpu
def test_whole_model_cfg3_batch128_256(cae):
    from cnn_autoencoder_amd import synth
    codec, eb = _canonical_codec(cae)
    tiles = np.concatenate([synth.histo_tiles(8, 256, first_index=100), synth.uniform_tiles(120, 256, seed=5)])
    host = codec.encode_batch(tiles)
    dev = codec.encode_batch(tiles, coder='device')
    assert dev == host
    assert np.array_equal(codec.decode_batch(dev, coder='device'), codec.decode_batch(host))


@gpu
def test_slide_run_device_matches_host(cae):
    from cnn_autoencoder_amd import slide, synth
    codec, eb = _canonical_codec(cae)
    tiles = torch.from_numpy(synth.histo_tiles(6, 256, first_index=40)).cuda()
    batches = [tiles[:4].contiguous(), tiles[2:].contiguous(), tiles[1:5].flip(1).contiguous()]
    stats_h, pay_h = slide.SlideCoder(codec).run(batches, keep_payloads=True)
    stats_d, pay_d = slide.SlideCoder(codec, coder='device').run(batches, keep_payloads=True)
    assert torch.equal(stats_h, stats_d)
    assert [list(p) for p in pay_h] == [list(p) for p in pay_d]
    sc = slide.SlideCoder(codec, coder='device')
    got = list(sc.compress_batches(batches))
    assert [list(p) for p in got] == [list(p) for p in pay_h]
    recs_d = [r.cpu() for r in sc.decompress_batches(got, 256, 256)]
    recs_h = [r.cpu() for r in slide.SlideCoder(codec).decompress_batches(got, 256, 256)]
    assert all(torch.equal(a, b) for a, b in zip(recs_d, recs_h))


@gpu
def test_slide_flow_device_chunks_identical(cae, tmp_path):
    from cnn_autoencoder_amd import synth, zarrio
    cfg = dict(synth.CANONICAL, channels_net=32, channels_bn=48, compression_level=3)
    ckpt = str(tmp_path / 'ckpt.pth')
    torch.save(synth.synthetic_state(cfg, seed=4), ckpt)
    img = synth.histo_tile(150, 3, 200)  # not a multiple of the 64-pixel patch
    a, b = str(tmp_path / 'host.zarr'), str(tmp_path / 'device.zarr')
    za = zarrio.compress_image('CAE', ckpt, img, a, patch_size=64, batch_tiles=5)
    zb = zarrio.compress_image('CAE', ckpt, img, b, patch_size=64, batch_tiles=5, coder='device')
    for idx in za.chunk_indices():
        assert za.read_chunk_bytes(idx) == zb.read_chunk_bytes(idx), idx
    rec_h = zarrio.decompress_image(a, batch_tiles=5)
    rec_d = zarrio.decompress_image(b, batch_tiles=5, coder='device')
    assert rec_d.shape == img.shape and np.array_equal(rec_d, rec_h)
