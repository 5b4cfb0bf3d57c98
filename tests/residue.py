"""Helpers for the tests that ask whether a result depends on what its buffers held before the call (no tests here).

poisoned_alloc   fixture: torch.empty / torch.empty_like / Tensor.new_empty hand out memory filled with a poison pattern
                 (NaN for floats, 0x7FC0 for bfloat16, bytes 0x7F for integers); device tensors sit between two 4-KiB
                 guard bands of the same pattern.  A buffer that a kernel does not write completely shows its poison in
                 the result; a kernel that writes outside its buffer breaks a band, which check() compares as bytes.
                 torch.zeros and friends are left alone: a buffer that kernels accumulate into must come from them.
covering_shape   the shape of a "dirtying" call for tests/test_call_order.py: rows without unwritten pitch, every
                 dimension at least the clean call's, at least twice its bytes at every level.  A call that writes every
                 byte of a larger extent leaves no byte of the smaller call's buffers, or of its over-reads, untouched.
"""
import math
import sys

import pytest
import torch

GUARD_BYTES = 4096  # a multiple of 512 B: the interior keeps the alignment of the allocation that data_ptr() callers rely on
# the poison of each floating type as the bits of a quiet NaN, written through an integer view of the same width so that
# host and device hold the same bytes whatever their fill kernels make of a NaN
_NAN_BITS = {torch.float32: (torch.int32, 0x7FC00000), torch.float64: (torch.int64, 0x7FF8000000000000),
             torch.float16: (torch.int16, 0x7E00), torch.bfloat16: (torch.int16, 0x7FC0)}


def poison_(t):
    """fills `t` (any dense tensor) with the poison pattern of its dtype: NaN for float32 / float64 / float16, 0x7FC0 for
    bfloat16, bytes 0x7F for everything else"""
    if t.numel() == 0:
        return t
    if t.dtype in _NAN_BITS:
        as_int, bits = _NAN_BITS[t.dtype]
        t.view(as_int).fill_(bits)
    elif t.dtype == torch.bool:
        t.fill_(True)
    elif t.dtype.is_complex:
        torch.view_as_real(t).fill_(float('nan'))
    elif t.dtype.is_floating_point:  # 8-bit floats
        t.view(torch.uint8).fill_(0x7F)
    else:
        t.fill_(int.from_bytes(b'\x7f' * t.dtype.itemsize, 'little'))
    return t


def guard_pattern(dtype):
    """the bytes of one guard band of `dtype`, as a uint8 host tensor"""
    return poison_(torch_empty(GUARD_BYTES // dtype.itemsize, dtype=dtype)).view(torch.uint8)


torch_empty = torch.empty  # the real one, kept before any test patches it
_torch_empty_like = torch.empty_like
_tensor_new_empty = torch.Tensor.new_empty


class PoisonedAlloc:
    """state of the poisoned_alloc fixture: the recorded device allocations and their check"""

    def __init__(self):
        self.records = []  # (whole allocation, guard elements, interior elements, call site)
        self.count = 0     # tensors handed out, host ones included
        self.guard_host = False  # host tensors are poisoned only; True fences them too (the helper's own tests)

    # ---- the three replacements
    def _finish(self, proto, requires_grad, site):
        """`proto` came from the real function (shape, strides, dtype, device, pinning as asked for): poisons it if it
        lives on the host, else replaces it by the interior of a guarded, poisoned allocation of the same geometry"""
        self.count += 1
        host = proto.device.type == 'cpu'
        if proto.device.type == 'meta' or proto.layout != torch.strided:
            out = proto
        elif host and not self.guard_host:
            out = poison_(proto)
        else:
            shape, stride = tuple(proto.shape), tuple(proto.stride())
            extent = 0 if proto.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(shape, stride))
            g = GUARD_BYTES // proto.dtype.itemsize
            dtype, device, pinned = proto.dtype, proto.device, host and proto.is_pinned()
            del proto
            whole = poison_(torch_empty(extent + 2 * g, dtype=dtype, device=device, pin_memory=pinned))
            out = whole.as_strided(shape, stride, g)
            assert (out.data_ptr() - whole.data_ptr()) % 512 == 0
            self.records.append((whole, g, extent, site))
        return out.requires_grad_() if requires_grad else out

    def empty(self, *size, **kw):
        if kw.get('out') is not None:
            return torch_empty(*size, **kw)
        rg = kw.pop('requires_grad', False)
        return self._finish(torch_empty(*size, **kw), rg, _site())

    def empty_like(self, x, **kw):
        rg = kw.pop('requires_grad', False)
        return self._finish(_torch_empty_like(x, **kw), rg, _site())

    def new_empty(self, x, *size, **kw):
        rg = kw.pop('requires_grad', False)
        return self._finish(_tensor_new_empty(x, *size, **kw), rg, _site())

    # ---- the check
    def check(self, release=True):
        """every guard band of every device tensor handed out so far still holds the pattern, byte for byte.
        `release`: forget the checked allocations (their memory returns to the allocator once the caller drops them)"""
        if self.records and self.records[0][0].is_cuda:
            torch.cuda.synchronize()
        patterns, broken = {}, []
        for whole, g, extent, site in self.records:
            key = (whole.dtype, whole.device)
            if key not in patterns:
                patterns[key] = guard_pattern(whole.dtype).to(whole.device)
            for name, band in (('below', whole[:g]), ('above', whole[g + extent:])):
                got = band.view(torch.uint8)
                if not torch.equal(got, patterns[key]):
                    at = int((got != patterns[key]).nonzero()[0 if name == 'above' else -1])
                    off = at if name == 'above' else at - GUARD_BYTES
                    broken.append(f'{site}: {extent} x {whole.dtype} written {name} the buffer '
                                  f'(byte {off:+d} from its {"end" if name == "above" else "start"})')
        checked = len(self.records)
        if release:
            self.records = []
        assert not broken, 'writes outside a buffer:\n' + '\n'.join(broken)
        return checked


def _site():
    """file:line of the caller of the patched function (skipping this module)"""
    f = sys._getframe(2)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    return 'unknown' if f is None else f'{f.f_code.co_filename.rsplit("/", 1)[-1]}:{f.f_lineno}'


@pytest.fixture
def poisoned_alloc(monkeypatch):
    pa = PoisonedAlloc()
    monkeypatch.setattr(torch, 'empty', pa.empty)
    monkeypatch.setattr(torch, 'empty_like', pa.empty_like)
    monkeypatch.setattr(torch.Tensor, 'new_empty', lambda self, *size, **kw: pa.new_empty(self, *size, **kw))
    yield pa
    pa.records = []


# --------------------------------------------------------------------------------------------- covering shapes
def pitch_c8(w):
    """fp32 C8 rows: 32 B per pixel, no slack"""
    return w * 32


def pitch_c8s(w):
    """C8S rows (analysis track, f16x3): whole 32-pixel groups of 1 KiB"""
    return math.ceil(w / 32) * 1024


def pitch_c8sp(w):
    """C8SP rows (synthesis track, f16x3): whole 64-pixel blocks of 2 KiB"""
    return math.ceil(w / 64) * 2048


PITCHES = (('C8', pitch_c8, 1), ('C8S', pitch_c8s, 32), ('C8SP', pitch_c8sp, 64))


def level_sizes(track, shape, levels):
    """[(rows, columns)] of the converted input and of every level's output: the analysis track halves (rounding up),
    the synthesis track doubles"""
    _, h, w = shape
    out = [(h, w)]
    for _ in range(levels):
        h, w = ((h + 1) // 2, (w + 1) // 2) if track == 'analysis' else (2 * h, 2 * w)
        out.append((h, w))
    return out


def assert_covers(track, clean_shape, dirty_shape, levels, kernel_size):
    """the three properties of a covering shape, at the converted input and at every level of the track"""
    assert track in ('analysis', 'synthesis'), track
    assert dirty_shape[0] == clean_shape[0], f'dirty n {dirty_shape[0]} != clean n {clean_shape[0]}'
    n = clean_shape[0]
    # fp32 path: C8 rows on both tracks; f16x3 path: C8S rows on the analysis track, C8SP rows on the synthesis track
    layouts = PITCHES[:2] if track == 'analysis' else (PITCHES[0], PITCHES[2])
    clean, dirty = level_sizes(track, clean_shape, levels), level_sizes(track, dirty_shape, levels)
    for lvl, ((ch, cw), (dh, dw)) in enumerate(zip(clean, dirty)):
        assert dh >= ch and dw >= cw, f'level {lvl}: dirty {dh} x {dw} is smaller than clean {ch} x {cw}'
        assert min(dh, dw) > kernel_size // 2, f'level {lvl}: dirty {dh} x {dw} is not above the padding'
        for name, pitch, group in layouts:
            assert dw % group == 0 and pitch(dw) == dw * 32, \
                f'level {lvl}: {name} rows of width {dw} have unwritten pitch ({pitch(dw)} B for {dw * 32} B of pixels)'
            # (the plane count is the model's, the same in both calls)
            assert n * dh * pitch(dw) >= 2 * n * ch * pitch(cw), \
                f'level {lvl}: {name} extent {n * dh * pitch(dw)} B is less than twice the clean {n * ch * pitch(cw)} B'


def covering_shape(track, clean_shape, levels, kernel_size, dirty=None):
    """-> (n, h, w) of a dirtying call for the clean call (n, h, w) (image size on the analysis track, latent size on
    the synthesis track) of a track of `levels` units with k = `kernel_size`: same n; no unwritten pitch at any level;
    every dimension at least the clean one; at least twice the clean call's bytes at every level.  `dirty` proposes a
    shape instead of the one worked out here; it is held to the same assertions."""
    n, h, w = clean_shape
    if dirty is None:
        if track == 'analysis':
            # sizes halve rounding up: whole groups of 32 * 2^levels columns keep every level a multiple of 32, and
            # 2^(levels + 1) ceil(h / 2^levels) rows are at every level twice ceil(h / 2^level)
            unit = 32 << levels
            dirty = (n, (2 << levels) * math.ceil(h / (1 << levels)), math.ceil(w / unit) * unit)
        else:
            # sizes double: a multiple of 64 stays one; twice the rows give twice the bytes whatever the widths
            dirty = (n, 2 * h, math.ceil(w / 64) * 64)
    dirty = tuple(int(v) for v in dirty)
    assert_covers(track, clean_shape, dirty, levels, kernel_size)
    return dirty
