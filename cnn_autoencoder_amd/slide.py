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
        self._pinned = {}
        self._busy = {}  # pinned buffer key -> event of the asynchronous copy that is still reading it
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

    # ---- device coder: kernels on a stream per batch in flight, called from worker threads ----------------------
    def _coder_stream(self, k):
        if self._coder_streams is None:
            self._coder_streams = [torch.cuda.Stream(_dev()) for _ in range(max(1, self.depth))]
        return self._coder_streams[k % len(self._coder_streams)]

    def _device_encode(self, k, sym):
        """symbols of batch k (complete: the caller has waited for them) -> PackedStreams on the host"""
        with torch.cuda.device(sym.device), torch.cuda.stream(self._coder_stream(k)):
            return self.eb.encode_symbols_device(sym)

    def _device_decode(self, k, payloads, hw):
        """payloads -> (n, C, hw) int32 symbols in HBM, complete when this returns (allocated on the coder stream)"""
        with torch.cuda.device(_dev()), torch.cuda.stream(self._coder_stream(k)):
            return self.eb.decode_symbols_device(payloads, hw)

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

    # ---- pipelined one-way streams (what compress.py / decompress.py do: encode only, decode only) ------------
    def _to_device(self, batch, k, stream):
        """A (n,h,w,c) uint8 batch on the GPU: CUDA tensors pass through, host arrays go through a pinned staging
        buffer and an asynchronous H2D on `stream`.  -> (tensor, event | None)."""
        if isinstance(batch, torch.Tensor) and batch.is_cuda:
            return batch, None
        arr = batch.numpy() if isinstance(batch, torch.Tensor) else np.ascontiguousarray(batch)
        if arr.dtype != np.uint8 or arr.ndim != 4:
            raise ValueError(f'expected a (n,h,w,c) uint8 batch, got {arr.dtype} {arr.shape}')
        key = ('t', k % (self.depth + 1))
        pin = self._pin(key, arr.shape, torch.uint8)
        self._wait_free(key)  # the H2D that last read this staging buffer
        pin.numpy()[...] = arr
        with torch.cuda.stream(stream):
            dev = pin.to(_dev(), non_blocking=True)
            ev = torch.cuda.Event(blocking=True)
            ev.record(stream)
        self._busy[key] = ev
        return dev, ev

    def _redo_analysis(self, t, main):
        """f16x3 range guard, rare path: the analysis of batch `t` overflowed the f16 range -> repeat it on the fp32
        kernels.  Runs on the calling (worker) thread but on the MAIN stream, so the handle's workspace is used in
        stream order; returns the symbols once they are complete."""
        with torch.cuda.device(t.device), torch.cuda.stream(main):
            sym = self.enc.forward_u8_symbols(t, self.eb)  # guarded call: falls back to fp32 by itself
            done = torch.cuda.Event(blocking=True)
            done.record(main)
        done.synchronize()
        return sym

    def _redo_synthesis(self, payloads, h, w, main, scale=0):
        with torch.cuda.device(_dev()), torch.cuda.stream(main):
            return self.decompress(payloads, h, w, scale)  # guarded calls

    # (events are created with blocking=True: a host thread that waits for one sleeps instead of spinning on a core --
    #  on a CPU share of 16 per GPU the spinning waiters took cycles from the coder pools)
    def _h2d_stream(self):
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(_dev())
        return self._copy_stream

    def _wait_free(self, key):
        ev = self._busy.pop(key, None)
        if ev is not None:
            ev.synchronize()

    @torch.no_grad()
    def compress_batches(self, batches):
        """Generator: for every (n,h,w,c) uint8 batch (CUDA tensor or host array) the list of rANS payloads (without
        the 16-byte chunk header), in order.  The GPU analyses up to `depth` batches ahead while a host worker pulls
        the symbols over the DMA engines and range-encodes them."""
        from concurrent.futures import ThreadPoolExecutor
        from . import _lib
        main = torch.cuda.current_stream(_dev())
        up = self._h2d_stream()
        depth = self.depth

        def stage(k, batch):
            t, ev = self._to_device(batch, k, up)
            if ev is not None:
                main.wait_event(ev)
                t.record_stream(main)
            sym, guard = self.enc.forward_u8_symbols(t, self.eb, defer=True)
            n, C = sym.size(0), sym.size(1)
            hw = sym.numel() // (n * C)
            pin = None if self.coder == 'device' else self._pin(('a', k % (depth + 1)), (n, C, hw), torch.int32)
            ready = torch.cuda.Event(blocking=True)
            ready.record(main)
            return pin, ready, sym, guard, t

        def pull(pin, ready, sym, guard, t):  # worker 1: DMA-engine D2H of batch k+1 while worker 2 encodes batch k
            ready.synchronize()
            if guard.overflowed():
                sym = self._redo_analysis(t, main)
            _lib.check(_lib.lib().cae_copy_to_host(pin.data_ptr(), sym.data_ptr(), sym.numel() * 4))
            return pin

        def encode(pulled):
            return self.eb.encode_symbols(pulled.result().numpy(), self.encode_threads)

        def device_encode(k, pin, ready, sym, guard, t):  # one worker per batch in flight, each on a coder stream
            ready.synchronize()
            if guard.overflowed():
                sym = self._redo_analysis(t, main)
            return self._device_encode(k, sym)

        device = self.coder == 'device'
        with ThreadPoolExecutor(max_workers=1) as d2h_pool, ThreadPoolExecutor(max_workers=depth if device else 1) as pool:
            inflight = []
            for k, batch in enumerate(batches):
                if device:
                    inflight.append(pool.submit(device_encode, k, *stage(k, batch)))
                else:
                    inflight.append(pool.submit(encode, d2h_pool.submit(pull, *stage(k, batch))))
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
        C = self.eb.channels

        device = self.coder == 'device'

        def decode(k, payloads):
            if device:  # symbols straight into HBM; complete when this returns
                return None, self._device_decode(k, payloads, lh * lw)
            key = ('d', k % (depth + 2))
            back = self._pin(key, (len(payloads), C, lh * lw), torch.int32)
            self._wait_free(key)  # the H2D that last read this buffer
            self.eb.decode_symbols(payloads, lh * lw, self.decode_threads, out=back.numpy())
            return key, back

        def synth(item):
            key, back = item
            if device:
                sym = back
            else:
                with torch.cuda.stream(up):
                    sym = back.to(_dev(), non_blocking=True)
                    ev = torch.cuda.Event(blocking=True)
                    ev.record(up)
                self._busy[key] = ev
                main.wait_event(ev)
            sym.record_stream(main)
            rec, guard = self.dec.forward_symbols_u8(sym.reshape(sym.size(0), C, lh, lw), self.eb, defer=True, scale=scale)
            done = torch.cuda.Event(blocking=True)
            done.record(main)
            return rec, guard, done

        def checked(rec, guard, done, payloads):
            """the reconstruction once it is complete and known to be in range (f16x3 guard; rare fp32 repeat)"""
            done.synchronize()
            if guard.overflowed():
                rec = self._redo_synthesis(payloads, h, w, main, scale)
                torch.cuda.current_stream(rec.device).synchronize()
            return rec

        def fetch(j, rec, guard, done, payloads):
            out = self._pin(('o', j % 4), tuple(rec.shape), torch.uint8)
            rec = checked(rec, guard, done, payloads)
            _lib.check(_lib.lib().cae_copy_to_host(out.data_ptr(), rec.data_ptr(), rec.numel()))
            return out.numpy()

        with ThreadPoolExecutor(max_workers=depth if device else 1) as pool, ThreadPoolExecutor(max_workers=1) as out_pool:
            inflight, outgoing, held, j = [], [], [], 0

            def emit(item, payloads):
                nonlocal j
                rec, guard, done = synth(item)
                if not to_host:
                    # one reconstruction is held back: its range check waits for its kernels, which run under the
                    # next batch's launch work instead of stalling the stream
                    held.append((rec, guard, done, payloads))
                    return [checked(*held.pop(0))] if len(held) > 1 else []
                outgoing.append(out_pool.submit(fetch, j, rec, guard, done, payloads))
                j += 1
                # one reconstruction stays in flight: its D2H overlaps the next batch's synthesis
                return [outgoing.pop(0).result()] if len(outgoing) > 1 else []

            for k, payloads in enumerate(payload_batches):
                payloads = list(payloads)
                inflight.append((pool.submit(decode, k, payloads), payloads))
                if len(inflight) > depth:
                    fut, pl = inflight.pop(0)
                    yield from emit(fut.result(), pl)
            while inflight:
                fut, pl = inflight.pop(0)
                yield from emit(fut.result(), pl)
            while held:
                yield checked(*held.pop(0))
            while outgoing:
                yield outgoing.pop(0).result()

    # ---- pipelined slide pass ----------------------------------------------------------------
    def _pin(self, key, shape, dtype):
        buf = self._pinned.get(key)
        if buf is None or buf.shape != tuple(shape) or buf.dtype != dtype:
            buf = torch.empty(shape, dtype=dtype, pin_memory=True)
            self._pinned[key] = buf
        return buf

    @torch.no_grad()
    def run(self, batches: Sequence[torch.Tensor], keep_payloads: bool = False):
        """Round-trip every batch ((n,h,w,c) uint8 in HBM).  -> (stats (sum n, 3) float64 host tensor,
        payload lists if keep_payloads).  Work of batch k: A = analysis+quantise+D2H (GPU),
        B = rANS encode + decode (host worker), D = H2D+dequantise+synthesis+SSE (GPU)."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        from . import _lib
        dev = batches[0].device
        main = torch.cuda.current_stream(dev)
        copy_up = self._h2d_stream()  # H2D beside the kernels of the main stream; D2H runs on the DMA engines (HSA)
        K = len(batches)
        # analysis runs DEPTH batches ahead of synthesis: the host always has a batch to code, and the GPU has analysis
        # work while the first batch crosses the host (D2H + encode + decode + H2D ~ 1.8 steps)
        DEPTH = self.depth
        tm = dict(host_encode=0.0, host_decode=0.0, wait_host=0.0, d2h_copy=0.0)
        all_payloads, stats_parts = [], []
        # all pinned symbol buffers up front (hipHostMalloc of 100 MB costs ~10 ms: not inside the pipeline)
        device = self.coder == 'device'
        n0, h0, w0, _ = batches[0].shape
        lh0, lw0 = self.enc.latent_size(h0, w0)
        for j in range(0 if device else DEPTH + 2):
            self._pin(('a', j), (n0, self.eb.channels, lh0 * lw0), torch.int32)
        for j in range(0 if device else DEPTH + 2):
            self._pin(('d', j), (n0, self.eb.channels, lh0 * lw0), torch.int32)

        def stage_a(k):
            t = batches[k]
            # quantiser fused into the last layer's epilogue; range check deferred to the encode worker
            sym, guard = self.enc.forward_u8_symbols(t, self.eb, defer=True)
            n, C = sym.size(0), sym.size(1)
            hw = sym.numel() // (n * C)
            # (host coder: in use until encode(k) is done)
            pin = None if device else self._pin(('a', k % (DEPTH + 2)), (n, C, hw), torch.int32)
            ready = torch.cuda.Event(blocking=True)
            ready.record(main)
            return k, pin, ready, hw, sym, guard

        def host_pull(k, pin, ready, hw, sym, guard):
            # D2H on the DMA engines from a worker thread of its own (cae_copy_to_host): a hipMemcpyAsync here runs as a
            # blit kernel under PyTorch's HIP runtime and held the main stream up for the whole PCIe transfer; in the
            # encode worker the 2 ms of the copy were serial with the 4-7 ms of range coding and set the step time
            ready.synchronize()
            if guard.overflowed():  # f16x3 range guard: repeat this batch on the fp32 kernels
                sym = self._redo_analysis(batches[k], main)
            t0 = time.perf_counter()
            _lib.check(_lib.lib().cae_copy_to_host(pin.data_ptr(), sym.data_ptr(), sym.numel() * 4))
            tm['d2h_copy'] += time.perf_counter() - t0
            return k, pin, hw

        def host_encode(pull_future):
            k, pin, hw = pull_future.result()
            t0 = time.perf_counter()
            payloads = self.eb.encode_symbols(pin.numpy(), self.encode_threads, packed=not keep_payloads)
            return k, payloads, hw, pin.shape, time.perf_counter() - t0

        def host_decode(enc_future):
            k, payloads, hw, shape, te = enc_future.result()
            t1 = time.perf_counter()
            # decode straight into pinned memory; the set is free again once H2D(k) has run (DEPTH + 2 sets: the decode
            # worker may be DEPTH batches ahead of the synthesis whose H2D is still queued)
            back = self._pin(('d', k % (DEPTH + 2)), shape, torch.int32)
            self.eb.decode_symbols(payloads, hw, self.decode_threads, out=back.numpy())
            return payloads, back, te, time.perf_counter() - t1

        # device coder: the same three stages with the symbols kept in HBM -- encode on batch k's coder stream, the bytes
        # D2H, back H2D and decode on that stream; one worker per batch in flight in each stage
        def device_encode(k, pin, ready, hw, sym, guard):
            ready.synchronize()
            if guard.overflowed():
                sym = self._redo_analysis(batches[k], main)
            t0 = time.perf_counter()
            payloads = self._device_encode(k, sym)
            return k, payloads, hw, tuple(sym.shape), time.perf_counter() - t0

        def device_decode(enc_future):
            k, payloads, hw, shape, te = enc_future.result()
            t1 = time.perf_counter()
            sym = self._device_decode(k, payloads, hw)
            return payloads, sym, te, time.perf_counter() - t1

        def stage_d(k, payloads, back):
            t = batches[k]
            n, h, w, c = t.shape
            if device:
                sym = back  # decoded into HBM, complete
            else:
                with torch.cuda.stream(copy_up):  # H2D beside the kernels of the main stream
                    sym = back.to(dev, non_blocking=True)
                    up = torch.cuda.Event(blocking=True)
                    up.record(copy_up)
                main.wait_event(up)
            sym.record_stream(main)
            lh, lw = h // 2 ** self.level, w // 2 ** self.level
            # dequantiser fused into the layout conversion in front of the first synthesis layer
            rec, guard = self.dec.forward_symbols_u8(sym.reshape(n, self.eb.channels, lh, lw), self.eb, defer=True)
            sse = self.tile_sse(rec, t)
            # the per-tile errors go to the host on the copy stream, behind an event of their own: read with a plain
            # `.cpu()` on the main stream they queued behind whatever had been launched since (the next batch's kernels),
            # the main thread sat in that copy until the GPU had drained, and every step began with a ~0.2 ms idle gap
            got = torch.cuda.Event()
            got.record(main)
            sse_host = self._pin(('s', k % 4), (n,), torch.float64)  # (finalised two batches later: 4 sets)
            with torch.cuda.stream(copy_up):
                copy_up.wait_event(got)
                sse_host.copy_(sse, non_blocking=True)
                landed = torch.cuda.Event(blocking=True)
                landed.record(copy_up)
            sse.record_stream(copy_up)
            nbytes = ([payloads.nbytes(i) + 16 for i in range(len(payloads))] if hasattr(payloads, 'nbytes')
                      else [len(p) + 16 for p in payloads])
            return (sse_host, landed), nbytes, h * w * c, guard, (k, payloads)

        pending = []  # ((pinned sse, landed event), nbytes list, samples, range guard, (k, payloads))

        def finalize(entry):
            """statistics of a finished batch (its range check needs its kernels done: the `landed` event is behind them);
            done with a lag of two batches inside the loop, so the payload buffers are released as the run proceeds --
            released all at once after the loop they cost ~2 ms per batch of pure host time inside the timed region"""
            (sse_pinned, landed), nbytes, samples, guard, (k, payloads) = entry
            landed.synchronize()  # this batch's kernels and the copy of its errors are done (the range flag too)
            sse_host = sse_pinned.tolist()
            if guard.overflowed():  # f16x3 range guard: repeat this batch's synthesis on the fp32 kernels
                t = batches[k]
                rec = self._redo_synthesis(payloads, t.shape[1], t.shape[2], main)
                sse_host = self.tile_sse(rec, t).cpu().tolist()
            stats_parts.append(tile_stats(nbytes, sse_host, samples))

        # three host workers: batch k+2 is pulled while batch k+1 is range-encoded and batch k is decoded
        workers = DEPTH if device else 1
        with ThreadPoolExecutor(max_workers=1) as pull_pool, ThreadPoolExecutor(max_workers=workers) as enc_pool, \
                ThreadPoolExecutor(max_workers=workers) as dec_pool:
            futs = {}

            def submit(k):
                if device:
                    futs[k] = dec_pool.submit(device_decode, enc_pool.submit(device_encode, *stage_a(k)))
                else:
                    futs[k] = dec_pool.submit(host_decode, enc_pool.submit(host_encode, pull_pool.submit(host_pull, *stage_a(k))))

            for k in range(min(DEPTH, K)):
                submit(k)
            for k in range(K):
                if k + DEPTH < K:
                    submit(k + DEPTH)
                t0 = time.perf_counter()
                payloads, back, te, td = futs.pop(k).result()
                tm['wait_host'] += time.perf_counter() - t0
                tm['host_encode'] += te
                tm['host_decode'] += td
                pending.append(stage_d(k, payloads, back))
                if keep_payloads:
                    all_payloads.append(payloads)
                del payloads
                if len(pending) > 2:
                    finalize(pending.pop(0))
        while pending:
            finalize(pending.pop(0))
        self.timers = tm
        return torch.cat(stats_parts), all_payloads
