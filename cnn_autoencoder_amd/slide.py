"""Sharded whole-slide compress / decompress driver (one process per GPU).

The reference codes one zarr chunk per dask task, batch 1, on a single device
(``compress.py:121-128``, ``_autoencoders.py:544``).  Tiles are independent units, so a slide's
tiles are split into contiguous blocks over the ranks of a ``torch.distributed`` job with NO
data-path collective: every rank codes its own tiles (and would write its own chunk files).  The
only exchange is one ``all_gather`` (RCCL over xGMI on GPUs, gloo on CPU) of a fixed-width per-tile
statistics record from which every rank derives the slide's rate and distortion
(bpp = 8*bytes/(H*W) as ``test_cae.py:73``; PSNR from the float64 SSE, ``test_cae.py:60-68`` without
its uint8 wrap-around).
"""
from __future__ import annotations

import math
import time
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

STATS_WIDTH = 3  # per tile: [compressed bytes, sum of squared error, number of pixel samples]


def tile_range(rank: int, world: int, n_tiles: int) -> Tuple[int, int]:
    """Contiguous block [lo, hi) of rank `rank` in chunk raster order."""
    if not (0 <= rank < world) or n_tiles < 0:
        raise ValueError(f'bad partition request rank={rank} world={world} n_tiles={n_tiles}')
    base, rem = divmod(n_tiles, world)
    lo = rank * base + min(rank, rem)
    hi = lo + base + (1 if rank < rem else 0)
    return lo, hi


def tile_stats(nbytes: Sequence[int], sse: Sequence[float], n_samples: int) -> torch.Tensor:
    """(n_tiles, 3) float64 record; bytes and counts are exact in float64 below 2^53."""
    out = torch.empty((len(nbytes), STATS_WIDTH), dtype=torch.float64)
    out[:, 0] = torch.tensor(list(nbytes), dtype=torch.float64)
    out[:, 1] = torch.tensor(list(sse), dtype=torch.float64)
    out[:, 2] = float(n_samples)
    return out


def gather_stats(local: torch.Tensor, counts: Sequence[int] = None) -> torch.Tensor:
    """all_gather of per-tile records over the default process group -> (total_tiles, 3) on every rank.

    Ranks may hold different tile counts (ragged last block): records are padded to the largest
    count for the collective and trimmed afterwards.
    """
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return local.clone()
    world = dist.get_world_size()
    dev = local.device
    n_local = torch.tensor([local.shape[0]], dtype=torch.int64, device=dev)
    all_n = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(all_n, n_local)
    all_n = [int(t.item()) for t in all_n]
    width = max(all_n)
    padded = torch.zeros((width, STATS_WIDTH), dtype=torch.float64, device=dev)
    padded[:local.shape[0]] = local
    bufs = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(bufs, padded)
    return torch.cat([b[:n] for b, n in zip(bufs, all_n)], dim=0)


COUNTS_WIDTH = 6  # per tile: [tp, tn, fp, fn, p, tp_top] (segmenters.COUNT_KEYS)


def gather_counts(local: torch.Tensor) -> torch.Tensor:
    """gather_stats for the per-tile counts records of SlideCoder.segment_batches: (n_tiles, 6) int64 on this rank ->
    (total_tiles, 6) on every rank, in rank order.  Ragged tile counts are padded to the largest for the collective and
    trimmed afterwards."""
    import torch.distributed as dist
    local = torch.as_tensor(local)
    if local.dim() != 2 or local.shape[1] != COUNTS_WIDTH or local.dtype != torch.int64:
        raise ValueError(f'expected (n_tiles, {COUNTS_WIDTH}) int64 records, got {local.dtype} {tuple(local.shape)}')
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return local.clone()
    world = dist.get_world_size()
    dev = local.device
    n_local = torch.tensor([local.shape[0]], dtype=torch.int64, device=dev)
    all_n = [torch.zeros_like(n_local) for _ in range(world)]
    dist.all_gather(all_n, n_local)
    all_n = [int(t.item()) for t in all_n]
    padded = torch.zeros((max(all_n), COUNTS_WIDTH), dtype=torch.int64, device=dev)
    padded[:local.shape[0]] = local
    bufs = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(bufs, padded)
    return torch.cat([b[:n] for b, n in zip(bufs, all_n)], dim=0)


def reduce_histogram(local: torch.Tensor) -> torch.Tensor:
    """The slide's ROC histogram from this rank's (segmenters.roc_histogram, summed over the rank's batches): the int64
    sum over the ranks of the default process group when torch.distributed is initialised, `local` itself otherwise.
    Integers: exact in any order."""
    import torch.distributed as dist
    local = torch.as_tensor(local)
    if local.dtype != torch.int64:
        raise ValueError(f'expected an int64 histogram, got {local.dtype}')
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return local
    total = local.clone() if dist.get_backend() == 'nccl' else local.cpu().clone()  # gloo sums host tensors
    dist.all_reduce(total, op=dist.ReduceOp.SUM)
    return total.to(local.device)


def slide_summary(stats: torch.Tensor, pixels_per_tile: int) -> Dict[str, float]:
    """Slide-level rate / distortion from the gathered records."""
    s = stats.double().cpu()
    nbytes = float(s[:, 0].sum())
    sse = float(s[:, 1].sum())
    n = float(s[:, 2].sum())
    n_tiles = s.shape[0]
    mse = sse / max(n, 1.0)
    return dict(tiles=n_tiles, bytes=nbytes, bpp=8.0 * nbytes / max(n_tiles * pixels_per_tile, 1),
                mse=mse, rmse=math.sqrt(mse), psnr=(10.0 * math.log10(255.0 ** 2 / mse) if mse > 0 else float('inf')))


def _dev():
    from . import _lib
    return _lib.require_gpu()


class _PinnedRing:
    """A ring of pinned host buffers: slot ``k % slots`` serves batch k.  A slot remembers the event of the asynchronous
    copy that still reads it and is handed out again only when that copy is done."""

    def __init__(self, slots: int):
        self.slots = slots
        self._bufs = [None] * slots
        self._readers = [None] * slots

    def take(self, k: int, shape, dtype) -> torch.Tensor:
        """the buffer of batch k, free of its last reader; a changed shape or dtype allocates it anew"""
        i = k % self.slots
        reader, self._readers[i] = self._readers[i], None
        if reader is not None:
            reader.synchronize()
        buf = self._bufs[i]
        if buf is None or buf.shape != tuple(shape) or buf.dtype != dtype:
            buf = self._bufs[i] = torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
        return buf

    def read_by(self, k: int, event) -> None:
        """`event` is behind an asynchronous copy that reads the buffer of batch k"""
        self._readers[k % self.slots] = event


def _clock(tm, key, t0):
    """the seconds since `t0` go to a driver's timers: one list per key, since several workers may append at once"""
    if tm is not None:
        tm[key].append(time.perf_counter() - t0)


class SlideCoder:
    """Batched compress -> decompress of resident tile batches on this rank's GPU.

    ``run(batches)`` software-pipelines the batches: while the host range-codes batch k
    (worker thread, GIL released inside libcae_hip.so), the GPU already runs the analysis of batch
    k+1 and the synthesis of batch k-1.  Symbols cross PCIe through pinned buffers on a side stream.
    """

    def __init__(self, codec, coder_threads: int = 0, coder: str = 'host'):
        from .codec import _module
        from .entropy import check_coder
        self.codec = codec
        # 'device': the range coder runs as HIP kernels on streams of their own (one per batch in flight); symbols never
        # leave HBM, only the compressed bytes cross PCIe.  Same bytes, statistics and range guard as 'host'.
        self.coder = check_coder(coder)
        self._coder_streams = None
        self.enc = _module(codec._model['encoder'])
        self.dec = _module(codec._model['decoder'])
        self.eb = _module(codec._model['fact_ent'])
        self.level = len(self.dec.synthesis_track)
        self.coder_threads = coder_threads  # the unpipelined compress() / decompress(): one pool at a time
        # pipelined drivers: an encode pool and a decode pool work side by side (plus this thread, the copy workers and
        # the HIP runtime's own threads), so the CPU budget (cae_cpu_budget: affinity / cgroup quota / ranks per node) is
        # SPLIT between them -- decoding costs about twice as much per symbol (2.1 vs 1.1 ns on a Zen 5 core), so it
        # gets the larger share.  Exceeding a cgroup quota throttles the whole process, GPU feeder included.
        self.encode_threads, self.decode_threads = self._split_budget(coder_threads)
        import os
        self.depth = int(os.environ.get('CAE_PIPELINE_DEPTH', '3'))  # batches the analysis runs ahead of the synthesis in run()
        self._rings = {}  # name -> _PinnedRing, see _ring()
        self._copy_stream = None  # side stream of the H2D copies
        self.timers = {}

    @staticmethod
    def _split_budget(requested: int = 0):
        from . import _lib
        import os
        if requested and requested > 0:
            return requested, requested
        if os.environ.get('CAE_ENC_THREADS', '0') != '0' and os.environ.get('CAE_DEC_THREADS', '0') != '0':
            return int(os.environ['CAE_ENC_THREADS']), int(os.environ['CAE_DEC_THREADS'])  # (tuning experiments)
        # Measured on a 16-CPU share (EPYC 9575F, 32 tiles of 1024^2 per batch = 16 lockstep work items per pool,
        # profiles/r02_experiments.md): decoding costs about twice the CPU time of encoding (2.1 vs 1.1 ns per symbol and
        # core), so the decode pool gets one thread per work item and the encode pool half as many; 24 runnable
        # threads on 16 CPUs caused no cgroup throttling (about 11 CPUs busy on average), while pools of 5 + 8 left
        # the GPU waiting for the host.
        # Below 12 CPUs (tools/sweep_host_budget.sh, 8 CPUs, lockstep 4: 8 + 8 threads 2352 tiles/s, 4 + 8 2133, 3 + 5 / 2 + 6
        # 1800-2100): the host is the bottleneck anyway, so both pools may use every CPU -- whichever stage has work runs.
        budget = int(_lib.lib().cae_cpu_budget())
        dec = max(1, min(16, budget))
        enc = max(1, min(16, budget if budget < 12 else budget // 2))
        return enc, dec

    # ---- simple (unpipelined) entry points ---------------------------------------------------
    @torch.no_grad()
    def compress(self, tiles_dev: torch.Tensor) -> List[bytes]:
        """tiles_dev (n,h,w,c) uint8 in HBM -> rANS payloads (without the 16-byte chunk header)."""
        y = self.enc.forward_u8(tiles_dev)
        sym = self.eb.quantize_symbols(y)
        if self.coder == 'device':
            return list(self.eb.encode_symbols_device(sym))
        sym_host = sym.reshape(sym.size(0), sym.size(1), -1).cpu().numpy()
        return self.eb.encode_symbols(sym_host, self.coder_threads)

    @torch.no_grad()
    def decompress(self, payloads: Sequence[bytes], h: int, w: int, scale: int = 0) -> torch.Tensor:
        """payloads -> (n,h,w,c) uint8 in HBM; ``scale = s``: (n,h/2^s,w/2^s,c), the tiles at 1 / 2^s of the resolution
        (Synthesizer.forward_scale_u8)."""
        scale = self.dec._check_scale(scale)
        size = (h // 2 ** self.level, w // 2 ** self.level)
        y_q = self.eb.decompress(payloads, size, coder=self.coder)
        return self.dec.forward_scale_u8(y_q, scale) if scale else self.dec.forward_u8(y_q)

    @torch.no_grad()
    def tile_sse(self, rec: torch.Tensor, tiles: torch.Tensor) -> torch.Tensor:
        """per-tile sum of squared error of two (n,h,w,c) uint8 batches -> (n,) float64 on the GPU."""
        from . import _lib
        n = tiles.shape[0]
        rec, tiles = rec.contiguous(), tiles.contiguous()
        out = torch.empty(n, dtype=torch.float64, device=tiles.device)
        _lib.check(_lib.lib().cae_tile_sse(rec.data_ptr(), tiles.data_ptr(), n, tiles[0].numel(), out.data_ptr(),
                                           _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def roundtrip(self, tiles_dev: torch.Tensor) -> Tuple[List[bytes], torch.Tensor, torch.Tensor]:
        """-> (payloads, reconstructed tiles in HBM, (n,3) float64 stats on the host)."""
        n, h, w, c = tiles_dev.shape
        payloads = self.compress(tiles_dev)
        rec = self.decompress(payloads, h, w)
        sse = self.tile_sse(rec, tiles_dev).cpu()
        stats = tile_stats([len(p) + 16 for p in payloads], sse.tolist(), h * w * c)
        return payloads, rec, stats

    # ---- pinned rings and streams of the pipelined drivers ----------------------------------------------------
    def _ring(self, name: str) -> _PinnedRing:
        """The pinned ring `name`.  The slot counts are in batches; d = `depth`, the batches a driver works ahead."""
        d = self.depth
        slots = {
            # host tiles staged for their H2D (compress_batches): the batch being filled and the one before it, whose
            # H2D may still run
            't': 2,
            # symbols pulled from the GPU: taken when the analysis of batch k is launched, read until batch k is
            # encoded.  Both drivers launch batch k before they collect batch k-d, so k-d .. k are in use
            'a': d + 1,
            # decoded symbols: taken when the decode worker starts batch k, read until H2D(k) is done.  Both drivers hand
            # batch k to the worker before they issue H2D(k-d), so k-d .. k are in use; one more slot, and the worker
            # waits for H2D(k-d-2), done long ago, instead of H2D(k-d-1), issued a moment ago
            'd': d + 2,
            # reconstructions of decompress_batches(to_host=True): batch k stays valid until the generator has advanced
            # two more times, and by the end of the second advance the fetches of k+1 .. k+3 have been submitted
            'o': 4,
            # per-tile errors of run(): batch k is finalised with a lag of two batches, so k-2 and k-1 are still
            # pending when k takes its slot
            's': 3,
            # class maps of segment_batches(to_host=True): as 'o' -- batch k stays valid until the generator has advanced
            # two more times, one fetch is kept in flight
            'c': 4,
        }[name]
        ring = self._rings.get(name)
        if ring is None or ring.slots != slots:
            ring = self._rings[name] = _PinnedRing(slots)
        return ring

    # (events are created with blocking=True: a host thread that waits for one sleeps instead of spinning on a core --
    #  on a CPU share of 16 per GPU the spinning waiters took cycles from the coder pools)
    def _h2d_stream(self):
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(_dev())
        return self._copy_stream

    def _coder_stream(self, k):
        """device coder: kernels on a stream per batch in flight, called from worker threads"""
        if self._coder_streams is None:
            self._coder_streams = [torch.cuda.Stream(_dev()) for _ in range(max(1, self.depth))]
        return self._coder_streams[k % len(self._coder_streams)]

    # ---- the stages of the pipelined drivers ------------------------------------------------------------------
    # `main`: the stream of the analysis and synthesis kernels; `up`: the side stream of the H2D copies; `tm`: the
    # timers of run() (None: not timed).
    def _launch_analysis(self, k, t, main):
        """Launches the analysis of batch k ((n,h,w,c) uint8 in HBM).  -> (symbols, range ticket, event behind
        them, pinned slot the symbols will be pulled into | None with the device coder)."""
        # quantiser fused into the last layer's epilogue; range check deferred to the worker that waits for `ready`
        sym, guard = self.enc.forward_u8_symbols(t, self.eb, defer=True)
        n, C = sym.size(0), sym.size(1)
        pin = None if self.coder == 'device' else self._ring('a').take(k, (n, C, sym.numel() // (n * C)), torch.int32)
        ready = torch.cuda.Event(blocking=True)
        ready.record(main)
        return sym, guard, ready, pin

    def _in_range(self, out, guard, done, main):
        """`out` of a deferred call (None: the caller has let go of it) once the event `done` behind the call has passed
        and its range ticket has been asked; the result of the fp32 repeat if a value had left the f16 range."""
        done.synchronize()
        return self._repeat_fp32(guard, main) if guard.overflowed() else out

    def _repeat_fp32(self, guard, main):
        """f16x3 range guard, rare path: repeats the ticket's own call (same device tensors) on the fp32 kernels.  Runs on
        the calling thread, often a worker, but on the MAIN stream, so the handle's workspace is used in stream order;
        returns the result once it is complete."""
        with torch.cuda.device(main.device), torch.cuda.stream(main):
            out = guard.rerun()
            done = torch.cuda.Event(blocking=True)
            done.record(main)
        done.synchronize()
        return out

    def _pull(self, sym, guard, ready, pin, main, tm):
        """symbols of a launched analysis, complete and in range, pulled into their pinned slot"""
        from . import _lib
        sym = self._in_range(sym, guard, ready, main)
        # D2H on the DMA engines from a worker thread of its own (cae_copy_to_host): a hipMemcpyAsync here runs as a
        # blit kernel under PyTorch's HIP runtime and held the main stream up for the whole PCIe transfer; in the
        # encode worker the 2 ms of the copy were serial with the 4-7 ms of range coding and set the step time
        t0 = time.perf_counter()
        _lib.check(_lib.lib().cae_copy_to_host(pin.data_ptr(), sym.data_ptr(), sym.numel() * 4))
        _clock(tm, 'd2h_copy', t0)
        return pin

    def _host_encode(self, pulled, packed, tm):
        pin = pulled.result()
        t0 = time.perf_counter()
        payloads = self.eb.encode_symbols(pin.numpy(), self.encode_threads, packed=packed)
        _clock(tm, 'host_encode', t0)
        return payloads

    def _device_encode(self, k, sym, guard, ready, main, tm):
        """symbols of a launched analysis, complete and in range, coded on batch k's coder stream -> PackedStreams on
        the host"""
        sym = self._in_range(sym, guard, ready, main)
        t0 = time.perf_counter()
        with torch.cuda.device(sym.device), torch.cuda.stream(self._coder_stream(k)):
            payloads = self.eb.encode_symbols_device(sym)
        _clock(tm, 'host_encode', t0)
        return payloads

    def _encode_async(self, k, t, main, pull_pool, enc_pool, packed, tm=None):
        """Launches the analysis of batch k and hands its symbols to the workers.  -> future of the payloads.
        Host coder: one worker pulls batch k+1 over the DMA engines while the next one encodes batch k.  Device coder:
        the symbols stay in HBM, one worker per batch in flight, each on a coder stream (`pull_pool` is idle)."""
        sym, guard, ready, pin = self._launch_analysis(k, t, main)
        if self.coder == 'device':
            return enc_pool.submit(self._device_encode, k, sym, guard, ready, main, tm)
        pulled = pull_pool.submit(self._pull, sym, guard, ready, pin, main, tm)
        return enc_pool.submit(self._host_encode, pulled, packed, tm)

    def _decode(self, k, payloads, hw, tm=None):
        """payloads of batch k -> its (n,C,hw) int32 symbols: in a pinned slot that is free again once H2D(k) has run, or
        with the device coder in HBM (decoded on batch k's coder stream, complete when this returns)."""
        t0 = time.perf_counter()
        if self.coder == 'device':
            stream = self._coder_stream(k)
            with torch.cuda.device(stream.device), torch.cuda.stream(stream):
                sym = self.eb.decode_symbols_device(payloads, hw)
        else:
            sym = self._ring('d').take(k, (len(payloads), self.eb.channels, hw), torch.int32)
            self.eb.decode_symbols(payloads, hw, self.decode_threads, out=sym.numpy())
        _clock(tm, 'host_decode', t0)
        return sym

    def _launch_synthesis(self, k, sym, lh, lw, main, up, scale=0):
        """symbols of batch k as _decode left them -> H2D beside the kernels of the main stream, then the synthesis
        launched on it.  -> (reconstruction (n,h,w,c) uint8, range ticket)."""
        if self.coder != 'device':
            with torch.cuda.stream(up):
                sym = sym.to(main.device, non_blocking=True)
                copied = torch.cuda.Event(blocking=True)
                copied.record(up)
            self._ring('d').read_by(k, copied)
            main.wait_event(copied)
        sym.record_stream(main)
        # dequantiser fused into the layout conversion in front of the first synthesis layer
        return self.dec.forward_symbols_u8(sym.reshape(sym.size(0), self.eb.channels, lh, lw), self.eb, defer=True,
                                           scale=scale)

    # ---- pipelined one-way streams (what compress.py / decompress.py do: encode only, decode only) ------------
    def _to_device(self, batch, k, up, main):
        """A (n,h,w,c) uint8 batch on the GPU, ready for the main stream: CUDA tensors pass through, host arrays go
        through a pinned staging buffer and an asynchronous H2D on `up`."""
        if isinstance(batch, torch.Tensor) and batch.is_cuda:
            return batch
        arr = batch.numpy() if isinstance(batch, torch.Tensor) else np.ascontiguousarray(batch)
        if arr.dtype != np.uint8 or arr.ndim != 4:
            raise ValueError(f'expected a (n,h,w,c) uint8 batch, got {arr.dtype} {arr.shape}')
        pin = self._ring('t').take(k, arr.shape, torch.uint8)
        pin.numpy()[...] = arr
        with torch.cuda.stream(up):
            dev = pin.to(_dev(), non_blocking=True)
            copied = torch.cuda.Event(blocking=True)
            copied.record(up)
        self._ring('t').read_by(k, copied)
        main.wait_event(copied)
        dev.record_stream(main)
        return dev

    @torch.no_grad()
    def compress_batches(self, batches):
        """Generator: for every (n,h,w,c) uint8 batch (CUDA tensor or host array) the list of rANS payloads (without
        the 16-byte chunk header), in order.  The GPU analyses up to `depth` batches ahead while a host worker pulls
        the symbols over the DMA engines and range-encodes them."""
        from concurrent.futures import ThreadPoolExecutor
        main = torch.cuda.current_stream(_dev())
        up = self._h2d_stream()
        depth = self.depth
        workers = depth if self.coder == 'device' else 1
        with ThreadPoolExecutor(max_workers=1) as pull_pool, ThreadPoolExecutor(max_workers=workers) as enc_pool:
            inflight = []
            for k, batch in enumerate(batches):
                inflight.append(self._encode_async(k, self._to_device(batch, k, up, main), main, pull_pool, enc_pool,
                                                   packed=False))
                if len(inflight) > depth:
                    yield inflight.pop(0).result()
            while inflight:
                yield inflight.pop(0).result()

    @torch.no_grad()
    def decompress_batches(self, payload_batches, h: int, w: int, to_host: bool = False, scale: int = 0):
        """``scale = s``: reconstructions at 1 / 2^s of the resolution, (n,h/2^s,w/2^s,c) (Synthesizer.forward_scale_u8).
        Generator: for every list of rANS payloads (tiles of h x w pixels) the (n,h,w,c) uint8 reconstruction, in
        order: a CUDA tensor, or with ``to_host`` a numpy array in a pinned ring buffer that stays valid until the
        generator has advanced two more times.  A host worker range-decodes up to `depth` batches ahead into pinned
        memory, H2D runs on a side stream beside the synthesis kernels, and with ``to_host`` a second worker pulls
        each reconstruction over the DMA engines while the next batch is synthesised."""
        from concurrent.futures import ThreadPoolExecutor
        from . import _lib
        scale = self.dec._check_scale(scale)
        main = torch.cuda.current_stream(_dev())
        up = self._h2d_stream()
        depth = self.depth
        lh, lw = h // 2 ** self.level, w // 2 ** self.level

        def fetch(k, rec, guard, done):
            out = self._ring('o').take(k, tuple(rec.shape), torch.uint8)
            rec = self._in_range(rec, guard, done, main)
            _lib.check(_lib.lib().cae_copy_to_host(out.data_ptr(), rec.data_ptr(), rec.numel()))
            return out.numpy()

        workers = depth if self.coder == 'device' else 1
        with ThreadPoolExecutor(max_workers=workers) as pool, ThreadPoolExecutor(max_workers=1) as out_pool:
            inflight, outgoing, held = [], [], []

            def emit(k, sym):
                rec, guard = self._launch_synthesis(k, sym, lh, lw, main, up, scale)
                done = torch.cuda.Event(blocking=True)
                done.record(main)
                if not to_host:
                    # one reconstruction is held back: its range check waits for its kernels, which run under the
                    # next batch's launch work instead of stalling the stream
                    held.append((rec, guard, done, main))
                    return [self._in_range(*held.pop(0))] if len(held) > 1 else []
                outgoing.append(out_pool.submit(fetch, k, rec, guard, done))
                # one reconstruction stays in flight: its D2H overlaps the next batch's synthesis
                return [outgoing.pop(0).result()] if len(outgoing) > 1 else []

            for k, payloads in enumerate(payload_batches):
                inflight.append((k, pool.submit(self._decode, k, list(payloads), lh * lw)))
                if len(inflight) > depth:
                    j, fut = inflight.pop(0)
                    yield from emit(j, fut.result())
            while inflight:
                j, fut = inflight.pop(0)
                yield from emit(j, fut.result())
            while held:
                yield self._in_range(*held.pop(0))
            while outgoing:
                yield outgoing.pop(0).result()

    # ---- pipelined slide pass ----------------------------------------------------------------
    @torch.no_grad()
    def run(self, batches: Sequence[torch.Tensor], keep_payloads: bool = False):
        """Round-trip every batch ((n,h,w,c) uint8 in HBM).  -> (stats (sum n, 3) float64 host tensor,
        payload lists if keep_payloads).  Work of batch k: A = analysis+quantise+D2H (GPU),
        B = rANS encode + decode (host worker), D = H2D+dequantise+synthesis+SSE (GPU)."""
        from concurrent.futures import ThreadPoolExecutor
        main = torch.cuda.current_stream(batches[0].device)
        copy_up = self._h2d_stream()  # H2D beside the kernels of the main stream; D2H runs on the DMA engines (HSA)
        K = len(batches)
        # analysis runs DEPTH batches ahead of synthesis: the host always has a batch to code, and the GPU has analysis
        # work while the first batch crosses the host (D2H + encode + decode + H2D ~ 1.8 steps)
        DEPTH = self.depth
        tm = {key: [] for key in ('host_encode', 'host_decode', 'wait_host', 'd2h_copy')}
        all_payloads, stats_parts = [], []
        device = self.coder == 'device'
        # all pinned symbol buffers up front (hipHostMalloc of 100 MB costs ~10 ms: not inside the pipeline)
        n0, h0, w0, _ = batches[0].shape
        lh0, lw0 = self.enc.latent_size(h0, w0)
        for ring in ([] if device else [self._ring('a'), self._ring('d')]):
            for j in range(ring.slots):
                ring.take(j, (n0, self.eb.channels, lh0 * lw0), torch.int32)

        def decode(k, encoded, hw):
            payloads = encoded.result()
            return payloads, self._decode(k, payloads, hw, tm)

        def stage_d(k, payloads, sym):
            t = batches[k]
            n, h, w, c = t.shape
            rec, guard = self._launch_synthesis(k, sym, h // 2 ** self.level, w // 2 ** self.level, main, copy_up)
            sse = self.tile_sse(rec, t)
            # the per-tile errors go to the host on the copy stream, behind an event of their own: read with a plain
            # `.cpu()` on the main stream they queued behind whatever had been launched since (the next batch's kernels),
            # the main thread sat in that copy until the GPU had drained, and every step began with a ~0.2 ms idle gap
            got = torch.cuda.Event()
            got.record(main)
            sse_host = self._ring('s').take(k, (n,), torch.float64)
            with torch.cuda.stream(copy_up):
                copy_up.wait_event(got)
                sse_host.copy_(sse, non_blocking=True)
                landed = torch.cuda.Event(blocking=True)
                landed.record(copy_up)
            sse.record_stream(copy_up)
            nbytes = ([payloads.nbytes(i) + 16 for i in range(len(payloads))] if hasattr(payloads, 'nbytes')
                      else [len(p) + 16 for p in payloads])
            return k, sse_host, landed, guard, nbytes, h * w * c

        pending = []  # what stage_d returned, of the batches not yet finalised

        def finalize(k, sse_pinned, landed, guard, nbytes, samples):
            """statistics of a finished batch (its range check needs its kernels done: the `landed` event is behind them,
            and behind the copy of its errors), done with a lag of two batches, so that it does not wait for the GPU"""
            rec = self._in_range(None, guard, landed, main)
            sse_host = sse_pinned.tolist()
            if rec is not None:  # the synthesis was repeated on the fp32 kernels
                sse_host = self.tile_sse(rec, batches[k]).cpu().tolist()
            stats_parts.append(tile_stats(nbytes, sse_host, samples))

        # three host workers: batch k+2 is pulled while batch k+1 is range-encoded and batch k is decoded
        # (device coder: the same stages with the symbols kept in HBM -- encode on batch k's coder stream, the bytes D2H,
        # back H2D and decode on that stream; one worker per batch in flight in each stage)
        workers = DEPTH if device else 1
        with ThreadPoolExecutor(max_workers=1) as pull_pool, ThreadPoolExecutor(max_workers=workers) as enc_pool, \
                ThreadPoolExecutor(max_workers=workers) as dec_pool:
            futs = {}

            def submit(k):
                lh, lw = self.enc.latent_size(*batches[k].shape[1:3])
                encoded = self._encode_async(k, batches[k], main, pull_pool, enc_pool, not keep_payloads, tm)
                futs[k] = dec_pool.submit(decode, k, encoded, lh * lw)

            for k in range(min(DEPTH, K)):
                submit(k)
            for k in range(K):
                if k + DEPTH < K:
                    submit(k + DEPTH)
                t0 = time.perf_counter()
                payloads, sym = futs.pop(k).result()
                _clock(tm, 'wait_host', t0)
                pending.append(stage_d(k, payloads, sym))
                if keep_payloads:
                    all_payloads.append(payloads)
                # the payload buffers are released as the run proceeds: released all at once after the loop they cost
                # ~2 ms per batch of pure host time inside the timed region
                del payloads
                if len(pending) > 2:
                    finalize(*pending.pop(0))
        while pending:
            finalize(*pending.pop(0))
        self.timers = {key: sum(spans) for key, spans in tm.items()}
        return torch.cat(stats_parts), all_payloads

    # ---- pipelined segmentation of compressed tiles ---------------------------------------------------------
    def segment_batches(self, payload_batches, h: int, w: int, seg_model, targets=None, threshold: float = 0.5,
                        threshold_on: str = 'scores', top_k: int = 5, scores: bool = False, keep_logits: bool = False,
                        to_host: bool = False, roc_bits=None, extents=None, object_level: bool = False, ap_bits=None):
        """Generator: for every list of chunk byte strings (the 16-byte '>QQ' tile size in front of the rANS payload, as
        ZarrArray.read_chunk_bytes returns and segmenters.segment_compressed takes them; tiles of h x w pixels) the
        prediction of the segmentation head ``seg_model`` (a JNet in eval mode), in order:
        dict(cls (n,h,w) uint8, scores (n,C,h,w) fp32 | None, counts (n,6) int64 | None, logits (n,C,h,w) | None).
        ``targets``: an iterable beside ``payload_batches`` of (n,h,w) uint8 label maps (host arrays or CUDA tensors);
        with it the counts are made (segmenters.predict).  Results are CUDA tensors, or with ``to_host`` numpy arrays;
        the class map then lies in a pinned ring buffer that stays valid until the generator has advanced two more times.
        ``roc_bits`` (8..14; one-class heads, needs ``targets``): each result gains 'roc_hist' (2, 2^roc_bits) int64, the
        batch's logit histograms of negatives and positives (segmenters.roc_histogram); ``extents``: an iterable beside
        the batches of (n, 2) integers (rows, cols), the part of each tile that the histogram counts.  A histogram is
        there to be summed over the slide (it adds exactly) and stays a CUDA tensor with ``to_host`` too.
        ``object_level`` (needs ``targets``): each result gains 'n_objects' (n,) int64, the connected objects of every
        label map (segmenters.components; by value for a head of several classes), and 'object_counts' (n,6) int64, the
        counts over the pixels of all object boxes (segmenters.object_cover, object_counts); with ``roc_bits`` also
        'object_roc_hist', the histogram over those pixels (segmenters.object_roc_histogram; stays on the device).
        ``extents`` then bound objects and boxes too.  All of it runs behind cae_seg_predict on the main stream, on the
        labels that are on the device already.
        ``ap_bits`` (8..14; needs ``targets``): each result gains 'ap_hist' (2, 2^ap_bits) int64 for
        segmenters.ap_from_histogram, counted inside ``extents`` and left on the device as 'roc_hist' is.  Several classes:
        the micro histogram of the batch's softmax scores (segmenters.score_histogram); the scores are made on the device
        for it whether or not ``scores`` asks to receive them.  One class: the logit histogram at ap_bits
        (segmenters.roc_histogram, read with key='logit'), the tensor of 'roc_hist' itself where ap_bits == roc_bits.

        The stages of decompress_batches: a worker range-decodes up to `depth` batches ahead (host or device coder), the
        symbols cross on the H2D side stream; then, on the main stream, dequantiser, synthesis track with its bridges
        (Synthesizer.forward), head, cae_seg_predict; with ``to_host`` a second worker pulls each class map over the
        DMA engines while the next batch runs.  A batch whose head call leaves the f16x3 range (FloatingPointError) is
        repeated on the head's fp32 torch ops; ``self.timers`` holds the seconds per stage and 'head_fp32_repeats'.

        ValueError before any work: seg_model in training mode, a head built for other latent channels than the
        codec's, a bad threshold / threshold_on / top_k, roc_bits without targets, for a head of several classes or
        outside 8..14, ap_bits without targets or outside 8..14, object_level without targets, extents without roc_bits,
        ap_bits or object_level; and for every batch,
        before it is handed to the decoder: a chunk whose header is not (h, w) -- chunks of mixed tile sizes."""
        from .codec import _module
        from . import segmenters
        seg = _module(seg_model)
        if seg.training:
            raise ValueError('segment_batches needs the head in eval mode: call seg_model.eval()')
        if seg._channels_bn != self.eb.channels:
            raise ValueError(f'the head expects {seg._channels_bn} latent channels (channels_bn), the codec has '
                             f'{self.eb.channels}')
        segmenters.threshold_logit(threshold, threshold_on)
        top_k = segmenters._check_top_k(top_k)
        if h % 2 ** self.level or w % 2 ** self.level:
            raise ValueError(f'tiles of {h} x {w} pixels are no multiple of 2^{self.level}')
        roc = None
        if roc_bits is not None:
            if targets is None:
                raise ValueError('roc_bits needs targets: the histograms are those of the labelled pixels')
            if seg._num_classes != 1:
                raise ValueError(f'roc_bits needs a one-class head, this one has {seg._num_classes} classes')
            roc = segmenters._check_roc_bits(roc_bits)
        ap = None
        if ap_bits is not None:
            if targets is None:
                raise ValueError('ap_bits needs targets: the histograms are those of the labelled pixels')
            if seg._num_classes > 255:
                raise ValueError(f'ap_bits takes heads of up to 255 classes, this one has {seg._num_classes}')
            ap = segmenters._check_ap_bits(ap_bits)
        if extents is not None and roc is None and ap is None and not object_level:
            raise ValueError('extents bound the histograms and the object boxes: they need roc_bits, ap_bits or '
                             'object_level')
        if object_level:
            if targets is None:
                raise ValueError('object_level needs targets: the objects are those of the label maps')
            segmenters._check_planes(1, int(h), int(w))
        return self._segment_batches(payload_batches, int(h), int(w), seg, targets,
                                     dict(threshold=threshold, threshold_on=threshold_on, top_k=top_k, scores=scores),
                                     keep_logits, to_host, roc, iter(extents) if extents is not None else None,
                                     bool(object_level), ap)

    @torch.no_grad()
    def _segment_batches(self, payload_batches, h, w, seg, targets, how, keep_logits, to_host, roc=None, extents=None,
                         object_level=False, ap=None):
        import struct
        from concurrent.futures import ThreadPoolExecutor
        from . import _lib, segmenters
        main = torch.cuda.current_stream(_dev())
        up = self._h2d_stream()
        depth = self.depth
        lh, lw = h // 2 ** self.level, w // 2 ** self.level
        head = struct.pack('>QQ', h, w)
        tm = {key: [] for key in ('host_decode', 'synthesis', 'head', 'predict', 'copy')}
        repeats = [0]
        targets = iter(targets) if targets is not None else None

        def strip(payloads):
            payloads = [bytes(p) for p in payloads]
            if any(p[:16] != head for p in payloads):
                raise ValueError(f'segment_batches needs chunks of one tile size, {h} x {w}: a chunk header differs')
            return [p[16:] for p in payloads]

        def fetch(k, res, done):
            done.synchronize()
            t0 = time.perf_counter()
            cls = res['cls']
            out = self._ring('c').take(k, tuple(cls.shape), torch.uint8)
            _lib.check(_lib.lib().cae_copy_to_host(out.data_ptr(), cls.data_ptr(), cls.numel()))
            # there to be summed: left on the device
            stay = {key: res[key] for key in ('roc_hist', 'object_roc_hist', 'ap_hist') if key in res}
            host = {key: None if v is None else v.cpu().numpy() for key, v in res.items() if key != 'cls' and key not in stay}
            _clock(tm, 'copy', t0)
            return dict(host, cls=out.numpy(), **stay)

        def launch(k, sym, target, extent):
            n = sym.size(0)
            if self.coder != 'device':
                with torch.cuda.stream(up):
                    sym = sym.to(main.device, non_blocking=True)
                    copied = torch.cuda.Event(blocking=True)
                    copied.record(up)
                self._ring('d').read_by(k, copied)
                main.wait_event(copied)
            sym.record_stream(main)
            t0 = time.perf_counter()
            y_q = self.eb.dequantize_symbols(sym.reshape(n, self.eb.channels, lh, lw))
            _, fx_brg = self.dec(y_q)  # range-guarded: synchronises, repeats itself on the fp32 kernels
            _clock(tm, 'synthesis', t0)
            t0 = time.perf_counter()
            try:
                logits = seg(y_q, fx_brg=fx_brg)[0]
            except FloatingPointError:  # f16x3 range of the head: its fp32 torch ops
                repeats[0] += 1
                logits = seg._forward_torch(y_q, list(fx_brg) if seg._concat_bridges else [])
            _clock(tm, 'head', t0)
            t0 = time.perf_counter()
            if target is not None and not (isinstance(target, torch.Tensor) and target.is_cuda):
                target = torch.as_tensor(np.ascontiguousarray(target)).to(main.device)
            several = ap is not None and seg._num_classes > 1  # the score histogram reads the scores of this call
            res = segmenters.predict(logits, target, **dict(how, scores=how['scores'] or several))
            res['logits'] = logits if keep_logits else None
            if extent is not None:  # on the device once, for every call below
                extent = segmenters._extent_arg(extent, n, main.device)
            if roc is not None:
                res['roc_hist'] = segmenters.roc_histogram(logits, target, extent=extent, bits=roc)
            if several:
                res['ap_hist'] = segmenters.score_histogram(res['scores'], target, extent=extent, bits=ap)
                if not how['scores']:
                    res['scores'] = None
            elif ap is not None:
                res['ap_hist'] = res['roc_hist'] if ap == roc else segmenters.roc_histogram(logits, target, extent=extent,
                                                                                            bits=ap)
            if object_level:
                labels, res['n_objects'] = segmenters.components(target.reshape(n, h, w), extent=extent,
                                                                 by_value=seg._num_classes > 1)
                cover = segmenters.object_cover(labels, extent=extent)
                res['object_counts'] = segmenters.object_counts(logits, target, cover, threshold=how['threshold'],
                                                                threshold_on=how['threshold_on'], top_k=how['top_k'])
                if roc is not None:
                    res['object_roc_hist'] = segmenters.object_roc_histogram(logits, target, cover, extent=extent, bits=roc)
            done = torch.cuda.Event(blocking=True)
            done.record(main)
            _clock(tm, 'predict', t0)
            return res, done

        workers = depth if self.coder == 'device' else 1
        try:
            with ThreadPoolExecutor(max_workers=workers) as pool, ThreadPoolExecutor(max_workers=1) as out_pool:
                inflight, outgoing = [], []

                def emit(j, fut, target, extent):
                    res, done = launch(j, fut.result(), target, extent)
                    if not to_host:
                        return [res]
                    outgoing.append(out_pool.submit(fetch, j, res, done))
                    # one class map stays in flight: its D2H overlaps the next batch's kernels
                    return [outgoing.pop(0).result()] if len(outgoing) > 1 else []

                for k, payloads in enumerate(payload_batches):
                    target = next(targets) if targets is not None else None
                    extent = next(extents) if extents is not None else None
                    inflight.append((k, pool.submit(self._decode, k, strip(payloads), lh * lw, tm), target, extent))
                    if len(inflight) > depth:
                        yield from emit(*inflight.pop(0))
                while inflight:
                    yield from emit(*inflight.pop(0))
                while outgoing:
                    yield outgoing.pop(0).result()
        finally:
            self.timers = dict({key: sum(spans) for key, spans in tm.items()}, head_fp32_repeats=repeats[0])
