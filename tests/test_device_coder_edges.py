"""The device rANS coder (csrc/cae_rans_device.hip) where test_device_coder.py does not reach: more than 1024 streams
(several streams per scan thread), CDF rows longer than one staging pass up to the 4096-entry limit, the 64-partition
cap of the count kernel, streams at unaligned addresses, the per-stream space verdicts, the codable-range boundary,
escape codes no encoder emits, and 256 damaged streams in one launch.  Everything is exact: the bytes are the host
coder's (and the oracle's), the verdict on a stream is the host decoder's on that stream alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cae_oracle as O
from test_device_coder import _Tables, _random_tables

OK, ARG, NOMEM, UNSUPPORTED, CORRUPT = 0, -1, -3, -4, -5
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def cae(built_lib):
    import cnn_autoencoder_amd as cae
    return cae


# ---- the raw ABI: caller-chosen buffers, offsets and sizes; the per-stream status comes back ---------------------------
def _workspace_bytes(t, n, hw):
    need = ctypes.c_size_t()
    t._lib.check(t._lib.lib().cae_rans_encode_workspace(t.h.ptr, n, hw, ctypes.byref(need)))
    return need.value


def _encode_raw(t, sym, out_capacity=None, ws_bytes=None, slack=256):
    """cae_rans_encode_device on buffers `slack` bytes larger than the sizes passed, the whole of them filled with a
    sentinel -> (status [n], offsets [n + 1], out bytes incl. the excess, workspace excess).  The default workspace holds
    ten words per symbol: a symbol takes 9 coder steps at the most."""
    sym = np.ascontiguousarray(sym, dtype=np.int32)
    n, hw = sym.shape[0], sym.shape[2]
    if ws_bytes is None:
        ws_bytes = 10 * _workspace_bytes(t, n, hw)
    if out_capacity is None:
        out_capacity = ws_bytes
    d_sym = torch.from_numpy(sym).cuda()
    ws = torch.full((ws_bytes + slack,), SENTINEL, dtype=torch.uint8, device='cuda')
    out = torch.full((out_capacity + slack,), SENTINEL, dtype=torch.uint8, device='cuda')
    offsets = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
    status = torch.full((n,), 99, dtype=torch.int32, device='cuda')
    t._lib.check(t._lib.lib().cae_rans_encode_device(t.h.ptr, d_sym.data_ptr(), n, hw, out.data_ptr(), out_capacity,
                                                     offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                                                     t._lib.stream_ptr()))
    torch.cuda.synchronize()
    return status.cpu().numpy(), offsets.cpu().numpy(), out.cpu().numpy(), ws[ws_bytes:].cpu().numpy()


def _stream(out, offsets, s):
    return out[offsets[s]:offsets[s + 1]].tobytes()


def _decode_raw(t, strings, hw, front=0, base=0):
    """cae_rans_decode_device on the streams packed back to back behind `front` junk bytes (offsets[0] = front), in a
    buffer that starts `base` bytes into an allocation -> (status [n], symbols (n, C, hw))"""
    n = len(strings)
    blob = bytes(range(1, front + 1)) + b''.join(strings)
    offsets = np.cumsum([front] + [len(s) for s in strings]).astype(np.int64)
    whole = torch.zeros(base + max(len(blob), 16), dtype=torch.uint8, device='cuda')
    buf = whole[base:]
    if blob:
        buf[:len(blob)].copy_(torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()))
    offs = torch.from_numpy(offsets).cuda()
    sym = torch.full((n, t.C, hw), -777, dtype=torch.int32, device='cuda')
    status = torch.full((n,), 99, dtype=torch.int32, device='cuda')
    t._lib.check(t._lib.lib().cae_rans_decode_device(t.h.ptr, buf.data_ptr(), len(blob), offs.data_ptr(), n, hw,
                                                     sym.data_ptr(), status.data_ptr(), t._lib.stream_ptr()))
    torch.cuda.synchronize()
    return status.cpu().numpy(), sym.cpu().numpy()


def _host_decode_verdicts(t, strings, hw):
    """the host decoder on every stream alone (cae_rans_decode_batch fails a whole batch on one bad stream) ->
    (status list, symbols or None per stream)"""
    status, symbols = [], []
    for s in strings:
        try:
            symbols.append(t.decode_host([s], hw)[0])
            status.append(OK)
        except t._lib.CaeError as e:
            assert 'error -5' in str(e)
            symbols.append(None)
            status.append(CORRUPT)
    return status, symbols


def _host_encode_verdicts(t, sym):
    status, strings = [], []
    for i in range(len(sym)):
        try:
            strings.append(t.encode_host(sym[i:i + 1])[0])
            status.append(OK)
        except ValueError as e:
            assert 'codable range' in str(e)
            strings.append(None)
            status.append(ARG)
    return status, strings


def _assert_device_decodes_as_host(t, strings, hw, host_status, host_symbols):
    status, sym = _decode_raw(t, strings, hw)
    assert status.tolist() == host_status
    for i, ref in enumerate(host_symbols):
        if ref is not None:
            assert np.array_equal(sym[i], ref), i


# ---- tables and symbols -----------------------------------------------------------------------------------------------
def _row(rng, entries, dominant=None):
    """a CDF row of `entries` entries: random frequencies, or one dominant symbol at index `dominant` among symbols of
    frequency 1 (they share LUT buckets: the decoder's forward scan runs long)"""
    bins = entries - 1
    if dominant is None:
        f = 1 + rng.multinomial(65536 - bins, rng.dirichlet(np.ones(bins)))
    else:
        f = np.ones(bins, dtype=np.int64)
        f[dominant] = 65536 - (bins - 1)
    return np.concatenate([[0], np.cumsum(f)]).astype(np.int32)


def _tables(rows, off):
    cdf = np.zeros((len(rows), max(len(r) for r in rows)), dtype=np.int32)
    for i, r in enumerate(rows):
        cdf[i, :len(r)] = r
    return _Tables(cdf, np.asarray([len(r) for r in rows], dtype=np.int32), np.asarray(off, dtype=np.int32))


def _symbols(rng, t, n, hw, beyond):
    """per channel uniform over the whole support and `beyond` values past either side of it"""
    cols = [rng.integers(int(t.off[c]) - beyond, int(t.off[c]) + int(t.lens[c]) - 2 + beyond, (n, 1, hw))
            for c in range(t.C)]
    return np.concatenate(cols, axis=1).astype(np.int32)


def _in_support(rng, t, n, hw):
    cols = [rng.integers(int(t.off[c]), int(t.off[c]) + int(t.lens[c]) - 2, (n, 1, hw)) for c in range(t.C)]
    return np.concatenate(cols, axis=1).astype(np.int32)


def _sprinkle_escapes(rng, t, sym, one_in):
    """about one symbol in `one_in` moved out of the support, by up to 3000"""
    esc = rng.random(sym.shape) < 1.0 / one_in
    far = rng.integers(1, 3000, sym.shape) * rng.choice([-1, 1], sym.shape)
    off = t.off.reshape(1, -1, 1)
    hi = (t.off + t.lens - 2).reshape(1, -1, 1)
    return np.where(esc, np.where(far < 0, off + far, hi + far - 1), sym).astype(np.int32)


# ---- without a device --------------------------------------------------------------------------------------------------
def test_rows_of_4097_entries_are_unsupported_at_every_entry_point(cae):
    from cnn_autoencoder_amd import _lib
    L = _lib.lib()
    fake = 1 << 20  # 16-byte aligned and never dereferenced: the shape check comes first
    size = ctypes.c_size_t()
    for stride, rc in ((4096, OK), (4097, UNSUPPORTED)):
        t = _Tables([[0, 32768, 65536] + [0] * (stride - 3)], [3], [0])
        assert L.cae_rans_encode_workspace(t.h.ptr, 4, 16, ctypes.byref(size)) == rc
        if rc == OK:
            continue
        assert '4096' in L.cae_last_error().decode()
        assert L.cae_rans_encode_device(t.h.ptr, fake, 4, 16, fake, 1 << 20, fake, fake, fake, 1 << 20, None) == rc
        assert L.cae_rans_decode_device(t.h.ptr, fake, 64, fake, 4, 16, fake, fake, None) == rc


# Escape codes no encoder emits: (name, the 4-bit values that follow the escape symbol, the stack ends there, the host's
# verdict).  The decoder adds up the count digits while they are 15, rejects a count above 8 (a 32-bit value has 8
# digits) and reads `count` digits, lowest first; it does not ask for the shortest code or for raw < 2^28.
_CRAFTED = (
    ('count 8, raw 0xFFFFFFFF', [8] + [15] * 8, False, OK),
    ('count 8', [8, 1, 7, 6, 5, 4, 3, 2, 8], False, OK),
    ('count 9', [9, 1, 2, 3, 4, 5, 6, 7, 8, 9], False, CORRUPT),
    ('15, 0', [15, 0], False, CORRUPT),
    ('15, 15, 1', [15, 15, 1], False, CORRUPT),
    ('15s to the end of the stream', [15] * 24, True, CORRUPT),
    ('count 7, raw >= 2^28', [7, 1, 2, 3, 4, 5, 6, 9], False, OK),
    ('count 3, raw 0', [3, 0, 0, 0], False, OK),
)
_CRAFTED_HW = 70


@functools.lru_cache(maxsize=None)
def _crafted_case():
    """(tables, streams, expected host status): every crafted code as the first, a middle and the last symbol of a
    stream of 3 x 70 symbols"""
    rng = np.random.default_rng(404)
    cdf, lens, off = _random_tables(rng, 3, 20)
    idx = np.repeat(np.arange(3), _CRAFTED_HW).tolist()
    strings, expect, stacks = [], [], []
    for name, code, ends, verdict in _CRAFTED:
        for pos in (0, 3 * _CRAFTED_HW // 2, 3 * _CRAFTED_HW - 1):
            sym = [int(off[c]) + int(rng.integers(-2, lens[c])) for c in idx]  # some ordinary escapes among them
            stack = []
            for i, c in enumerate(idx):
                if i != pos:
                    stack += O.rans_symbolize([sym[i]], [c], cdf.tolist(), lens.tolist(), off.tolist())
                    continue
                maxv = int(lens[c]) - 2
                stack.append((int(cdf[c, maxv]) & 0xFFFF, int(cdf[c, maxv + 1] - cdf[c, maxv]) & 0xFFFF, False))
                stack += [(d, d + 1, True) for d in code]
                if ends:
                    break
            strings.append(O.encode_stack(stack))
            expect.append(verdict)
    return (cdf, lens, off), strings, expect


def test_host_verdicts_on_crafted_escape_codes(cae):
    """the reference of the device test below, against the Python restatement of the upstream decoder where it accepts"""
    (cdf, lens, off), strings, expect = _crafted_case()
    t = _Tables(cdf, lens, off)
    status, symbols = _host_decode_verdicts(t, strings, _CRAFTED_HW)
    assert status == expect
    idx = np.repeat(np.arange(3), _CRAFTED_HW).tolist()
    for s, ref in zip(strings, symbols):
        if ref is not None:
            up = O.rans_decode_with_indexes(s, idx, cdf.tolist(), lens.tolist(), off.tolist())
            # (Python's integers do not wrap: raw 0xFFFFFFFF is -2^31 before the offset, an int32 after it)
            assert ref.reshape(-1).tolist() == [(v + 2 ** 31) % 2 ** 32 - 2 ** 31 for v in up]


_MUTATION_HW = 150


@functools.lru_cache(maxsize=None)
def _mutation_case(channels):
    """(tables, the 256 variants of one good stream): rows of up to 10 / 70 / 300 entries for 3 / 5 / 8 channels"""
    rng = np.random.default_rng(9040 + channels)  # (the host accepts 107 / 57 / 79 of the 256, 75 / 25 / 47 of them changed)
    tables = _random_tables(rng, channels, {3: 10, 5: 70, 8: 300}[channels])
    t = _Tables(*tables)
    sym = _sprinkle_escapes(rng, t, _in_support(rng, t, 1, _MUTATION_HW), 16)
    good = t.encode_host(sym)[0]
    variants = []
    for _ in range(128):  # single-bit flips
        b = bytearray(good)
        b[int(rng.integers(len(b)))] ^= 1 << int(rng.integers(8))
        variants.append(bytes(b))
    for _ in range(32):  # byte replacements
        b = bytearray(good)
        b[int(rng.integers(len(b)))] = int(rng.integers(256))
        variants.append(bytes(b))
    for _ in range(32):  # truncations to any length
        variants.append(good[:int(rng.integers(len(good)))])
    for _ in range(16):  # extensions by 1..9 bytes
        variants.append(good + rng.integers(0, 256, int(rng.integers(1, 10)), dtype=np.uint8).tobytes())
    for _ in range(16):  # word swaps
        w = np.frombuffer(good, dtype='<u4').copy()
        i, j = rng.choice(len(w), 2, replace=False)
        w[[i, j]] = w[[j, i]]
        variants.append(w.tobytes())
    for _ in range(16):  # zeroed tails
        k = int(rng.integers(1, len(good)))
        variants.append(good[:len(good) - k] + b'\x00' * k)
    variants += [good] * 16
    return tables, sym, variants


@pytest.mark.parametrize('channels', [3, 5, 8])
def test_host_accepts_and_rejects_enough_mutations(cae, channels):
    """the condition of the device test below: both verdicts are well represented among the 256"""
    tables, sym, variants = _mutation_case(channels)
    status, symbols = _host_decode_verdicts(_Tables(*tables), variants, _MUTATION_HW)
    assert len(variants) == 256
    assert status.count(OK) >= 40 and status.count(CORRUPT) >= 40
    assert all(np.array_equal(s, sym[0]) for s in symbols[-16:])


# ---- on the device ----------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize('n', [1024, 1025, 2049, 3000])
def test_more_than_1024_streams(cae, n):
    """each thread of the two scan kernels owns k = ceil(n / 1024) streams"""
    rng = np.random.default_rng(n)
    t = _Tables(*_random_tables(rng, 2, 12))
    sym = rng.integers(-12, 13, (n, 2, 5)).astype(np.int32)
    host = t.encode_host(sym)
    if n == 1025:
        assert host == [t.oracle_encode(sym[i]) for i in range(n)]
    status, offsets, out, _ = _encode_raw(t, sym)
    assert (status == OK).all()
    assert offsets.tolist() == np.cumsum([0] + [len(s) for s in host]).tolist()
    assert [_stream(out, offsets, s) for s in range(n)] == host
    status, back = _decode_raw(t, host, 5)
    assert (status == OK).all() and np.array_equal(back, sym)


@gpu
def test_one_uncodable_stream_among_2049(cae):
    rng = np.random.default_rng(1500)
    n, bad = 2049, 1500
    t = _Tables(*_random_tables(rng, 2, 12))
    sym = rng.integers(-12, 13, (n, 2, 5)).astype(np.int32)
    host = t.encode_host(sym)
    sym[bad, 1, 3] = 2 ** 29
    status, offsets, out, _ = _encode_raw(t, sym)
    assert status[bad] == ARG and (np.delete(status, bad) == OK).all()
    assert offsets[bad + 1] == offsets[bad]
    assert all(_stream(out, offsets, s) == host[s] for s in range(n) if s != bad)


@gpu
@pytest.mark.parametrize('case', ['mixed', 'all4096'])
def test_long_rows(cae, case):
    """rows of 65, 129, 1000 and 4096 entries (the LDS row staging loops), a row of one dominant symbol and 4094 symbols
    of frequency 1 (the decoder's scan within a LUT bucket runs long); symbols over the whole support and beyond"""
    rng = np.random.default_rng(65)
    if case == 'mixed':
        t = _tables([_row(rng, 65), _row(rng, 129), _row(rng, 1000), _row(rng, 4096), _row(rng, 4096, dominant=2000)],
                    [-8, 2, -500, -2047, 3])
    else:
        t = _tables([_row(rng, 4096), _row(rng, 4096, dominant=0), _row(rng, 4096)], [0, -4000, 7])
    n, hw = 65, 130
    sym = _symbols(rng, t, n, hw, 40)
    host = t.encode_host(sym)
    assert host[:3] == [t.oracle_encode(sym[i]) for i in range(3)]
    on_device = t.encode_device(sym)
    assert on_device == host
    assert np.array_equal(t.decode_device(host, hw), sym)
    assert np.array_equal(t.decode_host(on_device, hw), sym)


@gpu
@pytest.mark.parametrize('channels,hw', [(5, 209717), (3, 6000)])
def test_count_partitions(cae, channels, hw):
    """5 x 209717 = 1 048 585 symbols: the cap of 64 partitions, 16385 symbols each and the last one short; 3 x 6000: two.
    Escapes only in the last 100 symbols of stream 0 and the first 100 of stream 1: in one partition each"""
    rng = np.random.default_rng(hw)
    t = _Tables(*_random_tables(rng, channels, 40))
    sym = _in_support(rng, t, 2, hw)
    esc = _sprinkle_escapes(rng, t, sym, 2)
    flat, flat_esc = sym.reshape(2, -1), esc.reshape(2, -1)
    flat[0, -100:] = flat_esc[0, -100:]
    flat[1, :100] = flat_esc[1, :100]
    host = t.encode_host(sym)
    assert t.encode_device(sym) == host
    assert np.array_equal(t.decode_device(host, hw), sym)


@gpu
def test_unaligned_streams(cae):
    """streams that start 1, 2 and 3 bytes off a 4-byte boundary (the reader loads bytewise), by junk in front of them
    and by a buffer that itself starts off the boundary"""
    rng = np.random.default_rng(9)
    t = _Tables(*_random_tables(rng, 4, 30))
    sym = _sprinkle_escapes(rng, t, _in_support(rng, t, 9, 33), 8)
    host = t.encode_host(sym)
    status, aligned = _decode_raw(t, host, 33)
    assert (status == OK).all() and np.array_equal(aligned, sym)
    for shift in (1, 2, 3):
        for kw in (dict(front=shift), dict(base=shift)):
            status, back = _decode_raw(t, host, 33, **kw)
            assert (status == OK).all(), kw
            assert np.array_equal(back, aligned), kw


@gpu
def test_space_verdicts_output_capacity(cae):
    rng = np.random.default_rng(31)
    t = _Tables(*_random_tables(rng, 3, 30))
    sym = _sprinkle_escapes(rng, t, _in_support(rng, t, 9, 40), 8)
    host = t.encode_host(sym)
    ends = np.cumsum([len(s) for s in host])
    for capacity in (int(ends[-1]) - 4, int(ends[0]), int(ends[4]), int(ends[7])):
        status, offsets, out, ws_excess = _encode_raw(t, sym, out_capacity=capacity)
        fits = ends <= capacity  # the offsets are dense: stream s ends where the host's first s + 1 streams end
        assert status.tolist() == [OK if f else NOMEM for f in fits], capacity
        assert fits.any() and not fits.all()
        for s in np.flatnonzero(status == OK):
            assert offsets[s + 1] <= capacity and _stream(out, offsets, s) == host[s]
        assert (out[capacity:] == SENTINEL).all() and (ws_excess == SENTINEL).all()


@gpu
def test_space_verdicts_word_region(cae):
    """every symbol an escape of 1 or 2 digits (3 or 4 coder steps): the workspace of one word per symbol that
    cae_rans_encode_workspace gives holds the first two or three of nine streams"""
    rng = np.random.default_rng(32)
    t = _Tables(*_random_tables(rng, 3, 30))
    n, hw = 9, 40
    below = rng.random((n, 3, hw)) < 0.5
    far = rng.integers(1, 100, (n, 3, hw))
    sym = np.where(below, t.off.reshape(1, -1, 1) - far, (t.off + t.lens - 2).reshape(1, -1, 1) + far).astype(np.int32)
    host = t.encode_host(sym)
    ws_bytes = _workspace_bytes(t, n, hw)
    status, offsets, out, ws_excess = _encode_raw(t, sym, out_capacity=4 * ws_bytes, ws_bytes=ws_bytes)
    assert set(status.tolist()) == {OK, NOMEM}
    for s in np.flatnonzero(status == OK):
        assert _stream(out, offsets, s) == host[s]
    assert (out[4 * ws_bytes:] == SENTINEL).all() and (ws_excess == SENTINEL).all()
    # the Python wrapper doubles the workspace until every stream fits
    assert t.encode_device(sym) == host


@gpu
def test_range_boundary(cae):
    """one symbol at or beyond the codable range per stream, offsets 2 and -6 over an 11-symbol support: the device
    refuses exactly the streams the host refuses"""
    rng = np.random.default_rng(27)
    t = _tables([_row(rng, 13), _row(rng, 13)], [2, -6])
    p27, maxv = 2 ** 27, 11
    values = [p27, -p27, p27 + 1, p27 - 1, -p27 + 1, -p27 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 30 + 5, -2 ** 30 - 5]
    for off in (2, -6):  # raw = 2^28 - 1 | 2^28 + 1 below the support, raw = 2^28 - 2 | 2^28 above it
        values += [off - p27, off - p27 - 1, off + maxv + p27 - 1, off + maxv + p27]
    cases = [(v, c) for v in values for c in (0, 1)]
    sym = _in_support(rng, t, len(cases), 9)
    rule = []
    for i, (v, c) in enumerate(cases):
        sym[i, c, i % 9] = v
        value = v - int(t.off[c])
        raw = 0 if 0 <= value < maxv else (-2 * value - 1 if value < 0 else 2 * (value - maxv))
        rule.append(ARG if raw and (raw >= 2 ** 28 or abs(v) > p27) else OK)
    host_status, host = _host_encode_verdicts(t, sym)
    assert host_status == rule
    verdict = {v: host_status[i] for i, (v, c) in enumerate(cases) if c == 0}  # offset 2
    assert [verdict[p27], verdict[p27 + 1], verdict[-p27 + 2], verdict[-p27 + 1]] == [OK, ARG, OK, ARG]
    status, offsets, out, _ = _encode_raw(t, sym)
    assert status.tolist() == host_status
    assert all(_stream(out, offsets, i) == host[i] for i in range(len(cases)) if host[i] is not None)


@gpu
def test_crafted_escape_codes(cae):
    (cdf, lens, off), strings, expect = _crafted_case()
    t = _Tables(cdf, lens, off)
    host_status, host_symbols = _host_decode_verdicts(t, strings, _CRAFTED_HW)
    assert host_status == expect
    _assert_device_decodes_as_host(t, strings, _CRAFTED_HW, host_status, host_symbols)


@gpu
@pytest.mark.parametrize('channels', [3, 5, 8])
def test_256_mutations_in_one_launch(cae, channels):
    """bit flips, byte replacements, truncations, extensions, word swaps, zeroed tails and intact copies of one stream,
    packed back to back (the odd lengths put later streams at unaligned addresses) and decoded in one call"""
    tables, sym, variants = _mutation_case(channels)
    t = _Tables(*tables)
    host_status, host_symbols = _host_decode_verdicts(t, variants, _MUTATION_HW)
    assert host_status.count(OK) >= 40 and host_status.count(CORRUPT) >= 40
    _assert_device_decodes_as_host(t, variants, _MUTATION_HW, host_status, host_symbols)
