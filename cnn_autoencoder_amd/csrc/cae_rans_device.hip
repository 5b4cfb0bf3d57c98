// Device rANS coder of libcae_hip.so: the stream format of cae_entropy.cpp (one rANS64 stream per tile, 16-bit
// precision, 4-bit bypass escape) coded by HIP kernels, byte for byte what encode_streams / decode_streams write.
//
//   count    per stream the exact number of coder steps (count_steps): C*hw main steps plus the escape steps, which
//            are data-parallel -- a grid of (partition, stream) blocks sums them; out-of-range symbols flag the stream
//   scan     one workgroup: capacities steps + 2 words -> exclusive offsets into the word region, per-stream status
//   encode   ONE LANE PER STREAM, one wave per workgroup.  All lanes walk (c, i) from the last symbol to the first in
//            lock step, so the wave is on the same channel at the same time: the channel's EncSym row is staged in LDS
//            once per channel and the symbols in coalesced chunks of kChunk per lane.  Words go backwards from the end
//            of the stream's capacity region (plain vector stores), as the host writes them
//   compact  lengths -> dense byte offsets (scan) and one copy of every stream's words into a single byte buffer
//   decode   one lane per stream walking forward: LUT bucket + short scan in the LDS-staged CDF row; the symbols go
//            through an LDS tile to coalesced stores of the (n, C, hw) int32 output
// Every loop is bounded by C, hw, the row length and (decoder) 8 bypass digits; every read is bounds-checked against
// the stream's end.
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"

#include <algorithm>
#include <climits>
#include <cstring>

namespace cae {

namespace {

constexpr uint64_t kRansL = 1ull << 31;
constexpr uint32_t kPrecision = 16;
constexpr uint32_t kBypassBits = 4;
constexpr uint32_t kMaxBypass = (1u << kBypassBits) - 1;
constexpr int kLutBits = EntropyTables::kLutBits;
constexpr int kLanes = 64;                     // streams per workgroup (one wave)
constexpr int kChunk = 64;                     // symbols per lane staged in LDS at a time
constexpr int kStage = kLanes * (kChunk + 1);  // int32 words of the staging tile (row pitch 65: no bank conflicts)
constexpr int kScanThreads = 1024;
constexpr int kCountThreads = 256;
constexpr int kMaxStride = 4096;  // CDF row length the LDS-staged rows allow (24 B per EncSym)
constexpr int kMaxStreams = 65535;  // one grid row per stream in the count and compact kernels
constexpr int kStatusRange = CAE_ERR_ARG, kStatusSpace = CAE_ERR_NOMEM, kStatusCorrupt = CAE_ERR_CORRUPT;

using EncSym = EntropyTables::EncSym;
static_assert(sizeof(EncSym) == 24, "EncSym layout");

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// partitions of one stream's C*hw symbols in the count kernel
inline int count_parts(int C, int hw) {
    const size_t total = (size_t)C * hw;
    return (int)std::min<size_t>(64, std::max<size_t>(1, (total + 16383) / 16384));
}

// workspace of cae_rans_encode_device: [partial steps int64 n*P][partial flags int32 n*P][capacity offsets int64 n+1]
// [lengths in words int64 n] | 256-aligned word region (the rest)
struct EncLayout {
    size_t steps, flags, cap_off, lens, words;
    EncLayout(int n, int P) {
        steps = 0;
        flags = align_up(steps + (size_t)n * P * 8, 16);
        cap_off = align_up(flags + (size_t)n * P * 4, 16);
        lens = align_up(cap_off + (size_t)(n + 1) * 8, 16);
        words = align_up(lens + (size_t)n * 8, 256);
    }
};

// ---- kernels ---------------------------------------------------------------------------------------------------------

// escape steps of a block's share of one stream (count_steps); flags the stream when a symbol is outside the codable range
__global__ void __launch_bounds__(kCountThreads) rans_count_kernel(const int32_t *__restrict__ symbols,
                                                                   const int32_t *__restrict__ len,
                                                                   const int32_t *__restrict__ off, int C, int hw, int P,
                                                                   int64_t *__restrict__ part_steps,
                                                                   int32_t *__restrict__ part_flags) {
    const int s = blockIdx.y, p = blockIdx.x;
    const uint32_t total = (uint32_t)C * (uint32_t)hw;  // < 2^31 (checked by the host)
    const uint32_t per = (total + P - 1) / P;
    const uint32_t lo = (uint32_t)p * per, hi = min(total, lo + per);
    const int32_t *sym = symbols + (size_t)s * total;
    int64_t esc = 0;
    int bad = 0;
    for (uint32_t e = lo + threadIdx.x; e < hi; e += kCountThreads) {
        const int c = (int)(e / (uint32_t)hw);
        const int32_t v32 = sym[e];
        const int32_t o = off[c], maxv = len[c] - 2;
        const int64_t value = (int64_t)v32 - o;
        if (value >= 0 && value < maxv) continue;
        if (v32 > (1 << 27) || v32 < -(1 << 27)) {
            bad = 1;
            continue;
        }
        const uint64_t raw = value < 0 ? (uint64_t)(-2 * value - 1) : (uint64_t)(2 * (value - maxv));
        if (raw >= (1u << 28)) {
            bad = 1;
            continue;
        }
        int nb = 0;
        while (nb < 8 && (raw >> (nb * kBypassBits)) != 0) ++nb;  // <= 7 digits below 2^28
        esc += nb / (int)kMaxBypass + 1 + nb;
    }
    __shared__ int64_t red[kCountThreads];
    __shared__ int redf[kCountThreads];
    red[threadIdx.x] = esc;
    redf[threadIdx.x] = bad;
    __syncthreads();
    for (int w = kCountThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[threadIdx.x] += red[threadIdx.x + w];
            redf[threadIdx.x] |= redf[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part_steps[(size_t)s * P + p] = red[0];
        part_flags[(size_t)s * P + p] = redf[0];
    }
}

// exclusive scan of one value per thread over the kScanThreads threads of the block: thread t's base
__device__ int64_t block_exclusive_base(int64_t local) {
    __shared__ int64_t buf[kScanThreads];
    const int t = threadIdx.x;
    buf[t] = local;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int64_t add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    return buf[t] - local;
}

// capacity of stream s in words (0 when a symbol is outside the codable range)
__device__ __forceinline__ int64_t stream_capacity(const int64_t *part_steps, const int32_t *part_flags, int s, int P,
                                                   int64_t main_steps, int &bad) {
    int64_t esc = 0;
    bad = 0;
    for (int p = 0; p < P; ++p) {
        esc += part_steps[(size_t)s * P + p];
        bad |= part_flags[(size_t)s * P + p];
    }
    return bad ? 0 : main_steps + esc + 2;
}

// capacities steps + 2 words -> cap_off[0..n]; status per stream (range / word region too small).  Thread t owns the
// streams [t k, (t+1) k).
__global__ void __launch_bounds__(kScanThreads) rans_capacity_kernel(const int64_t *__restrict__ part_steps,
                                                                     const int32_t *__restrict__ part_flags, int n, int P,
                                                                     int64_t main_steps, int64_t region_words,
                                                                     int64_t *__restrict__ cap_off,
                                                                     int32_t *__restrict__ status) {
    const int k = (n + kScanThreads - 1) / kScanThreads;
    const int lo = min(n, (int)threadIdx.x * k), hi = min(n, lo + k);
    int bad;
    int64_t local = 0;
    for (int s = lo; s < hi; ++s) local += stream_capacity(part_steps, part_flags, s, P, main_steps, bad);
    int64_t run = block_exclusive_base(local);
    for (int s = lo; s < hi; ++s) {
        const int64_t cap = stream_capacity(part_steps, part_flags, s, P, main_steps, bad);
        cap_off[s] = run;
        run += cap;
        status[s] = bad ? kStatusRange : (run > region_words ? kStatusSpace : CAE_OK);
    }
    if ((int)threadIdx.x == kScanThreads - 1) cap_off[n] = run;
}

// Rans64EncPutBits(val, 4) onto the backwards writer; false when the capacity region is exhausted
__device__ __forceinline__ bool put_bits(uint64_t &x, uint32_t *__restrict__ words, int64_t &wp, int64_t lo,
                                         uint32_t val) {
    const uint64_t x_max = ((kRansL >> 16) << 32) * (uint64_t)(1u << (16 - kBypassBits));
    if (x >= x_max) {
        if (wp <= lo) return false;
        words[--wp] = (uint32_t)x;
        x >>= 32;
    }
    x = (x << kBypassBits) | val;
    return true;
}

__global__ void __launch_bounds__(kLanes) rans_encode_kernel(const EncSym *__restrict__ enc,
                                                             const int32_t *__restrict__ len,
                                                             const int32_t *__restrict__ off, int stride, int C, int hw,
                                                             int n, const int32_t *__restrict__ symbols,
                                                             const int64_t *__restrict__ cap_off,
                                                             uint32_t *__restrict__ words, int64_t *__restrict__ lens,
                                                             int32_t *__restrict__ status) {
    extern __shared__ __align__(16) unsigned char lds[];
    int32_t *stage = reinterpret_cast<int32_t *>(lds);                         // [kLanes][kChunk + 1]
    EncSym *row = reinterpret_cast<EncSym *>(lds + kStage * sizeof(int32_t));  // [stride]
    const int lane = threadIdx.x;
    const int s0 = blockIdx.x * kLanes;
    const int s = s0 + lane;
    bool active = s < n && status[s] == CAE_OK;
    bool overflow = false;
    const int64_t lo = s < n ? cap_off[s] : 0;
    const int64_t end = s < n ? cap_off[s + 1] : 0;
    int64_t wp = end;
    uint64_t x = kRansL;
    const size_t per = (size_t)C * hw;
    const int nchunks = (hw + kChunk - 1) / kChunk;
    // chunk t of the walk: channel C-1 - t / nchunks, chunk nchunks-1 - t % nchunks.  Its symbols are loaded into
    // registers (coalesced: element `lane` of every stream's chunk) while chunk t-1 is coded, then moved to LDS.
    int32_t pre[kLanes];
    auto load_chunk = [&](int t) {
        const int c = C - 1 - t / nchunks, base = (nchunks - 1 - t % nchunks) * kChunk;
        const int cnt = min(kChunk, hw - base);
#pragma unroll
        for (int r = 0; r < kLanes; ++r) {
            const int sr = s0 + r;
            pre[r] = (sr < n && lane < cnt) ? symbols[(size_t)sr * per + (size_t)c * hw + base + lane] : 0;
        }
    };
    load_chunk(0);
    const int steps = C * nchunks;
    for (int t = 0; t < steps; ++t) {
        const int c = C - 1 - t / nchunks, k = nchunks - 1 - t % nchunks;
        const int32_t o = off[c], maxv = len[c] - 2;
        const int base = k * kChunk;
        const int cnt = min(kChunk, hw - base);
        __syncthreads();  // the previous chunk (and row) are no longer read
#pragma unroll
        for (int r = 0; r < kLanes; ++r) stage[r * (kChunk + 1) + lane] = pre[r];
        if (k == nchunks - 1)
            for (int v = lane; v <= maxv; v += kLanes) row[v] = enc[(size_t)c * stride + v];
        __syncthreads();
        if (t + 1 < steps) load_chunk(t + 1);
        {
            if (!active) continue;
            const int32_t *mine = stage + lane * (kChunk + 1);
            for (int j = cnt - 1; j >= 0; --j) {
                const int32_t sym = mine[j];
                int32_t v = sym - o;
                if ((unsigned)v >= (unsigned)maxv) {  // escape (rare); the count kernel has checked the range
                    const uint32_t raw = v < 0 ? (uint32_t)(-2 * v - 1) : (uint32_t)(2 * (v - maxv));
                    v = maxv;
                    int nb = 0;
                    while (nb < 8 && (raw >> (nb * kBypassBits)) != 0) ++nb;
                    bool ok = true;
                    for (int d = nb - 1; d >= 0; --d)
                        ok = ok && put_bits(x, words, wp, lo, (raw >> (d * kBypassBits)) & kMaxBypass);
                    ok = ok && put_bits(x, words, wp, lo, (uint32_t)(nb % (int)kMaxBypass));
                    for (int q = 0; q < nb / (int)kMaxBypass; ++q) ok = ok && put_bits(x, words, wp, lo, kMaxBypass);
                    if (!ok) {
                        overflow = true;
                        break;
                    }
                }
                const EncSym e = row[v];
                const uint64_t x_max = ((kRansL >> kPrecision) << 32) * (uint64_t)e.freq;
                uint64_t xx = x;
                if (xx >= x_max) {
                    if (wp <= lo) {
                        overflow = true;
                        break;
                    }
                    words[--wp] = (uint32_t)xx;
                    xx >>= 32;
                }
                const uint64_t q = __umul64hi(xx, e.rcp_freq) >> e.rcp_shift;
                x = xx + e.bias + q * e.cmpl_freq;
            }
            if (overflow) active = false;
        }
    }
    if (s >= n) return;
    if (active && wp - lo >= 2) {
        words[--wp] = (uint32_t)(x >> 32);
        words[--wp] = (uint32_t)x;
        lens[s] = end - wp;
    } else {
        // (the capacity is exact: a region can only run out on a count / encode disagreement)
        if (active || overflow) status[s] = kStatusSpace;
        lens[s] = 0;
    }
}

// lengths (words) -> dense byte offsets of the packed output; status when the output buffer is too small
__global__ void __launch_bounds__(kScanThreads) rans_offsets_kernel(const int64_t *__restrict__ lens, int n,
                                                                    int64_t out_capacity, int64_t *__restrict__ offsets,
                                                                    int32_t *__restrict__ status) {
    const int k = (n + kScanThreads - 1) / kScanThreads;
    const int lo = min(n, (int)threadIdx.x * k), hi = min(n, lo + k);
    int64_t local = 0;
    for (int s = lo; s < hi; ++s) local += 4 * lens[s];
    int64_t run = block_exclusive_base(local);
    for (int s = lo; s < hi; ++s) {
        offsets[s] = run;
        run += 4 * lens[s];
        if (run > out_capacity && status[s] == CAE_OK) status[s] = kStatusSpace;
    }
    if ((int)threadIdx.x == kScanThreads - 1) offsets[n] = run;
}

__global__ void __launch_bounds__(256) rans_compact_kernel(const uint32_t *__restrict__ words,
                                                           const int64_t *__restrict__ cap_off,
                                                           const int64_t *__restrict__ lens,
                                                           const int64_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ status,
                                                           uint32_t *__restrict__ out) {
    const int s = blockIdx.y;
    if (status[s] != CAE_OK) return;
    const int64_t nw = lens[s];
    const uint32_t *src = words + (cap_off[s + 1] - nw);
    uint32_t *dst = out + offsets[s] / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}

// bounds-checked forward reader over one stream [p, end); the next kAhead words are loaded ahead (a shift register:
// one lane per stream leaves no other wave to hide the load latency behind)
constexpr int kAhead = 8;
struct DevReader {
    const unsigned char *base;
    int64_t p, end;
    bool aligned, bad;
    uint32_t ahead[kAhead];  // words at p, p + 4, ...
    __device__ __forceinline__ uint32_t load(int64_t q) const {
        if (q + 4 > end) return 0;
        if (aligned) return *reinterpret_cast<const uint32_t *>(base + q);
        return (uint32_t)base[q] | ((uint32_t)base[q + 1] << 8) | ((uint32_t)base[q + 2] << 16) |
               ((uint32_t)base[q + 3] << 24);
    }
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int i = 0; i < kAhead; ++i) ahead[i] = load(p + 4 * i);
    }
    __device__ __forceinline__ uint32_t next() {
        if (p + 4 > end) {
            bad = true;
            return 0;
        }
        const uint32_t w = ahead[0];
#pragma unroll
        for (int i = 0; i + 1 < kAhead; ++i) ahead[i] = ahead[i + 1];
        ahead[kAhead - 1] = load(p + 4 * kAhead);
        p += 4;
        return w;
    }
};

__device__ __forceinline__ uint32_t get_bits(uint64_t &x, DevReader &r) {
    const uint32_t val = (uint32_t)(x & kMaxBypass);
    x >>= kBypassBits;
    if (x < kRansL) x = (x << 32) | r.next();
    return val;
}

__global__ void __launch_bounds__(kLanes) rans_decode_kernel(const int32_t *__restrict__ cdf,
                                                             const uint16_t *__restrict__ lut,
                                                             const int32_t *__restrict__ len,
                                                             const int32_t *__restrict__ off, int stride, int C, int hw,
                                                             int n, const unsigned char *__restrict__ bytes,
                                                             int64_t bytes_len, const int64_t *__restrict__ offsets,
                                                             int32_t *__restrict__ symbols, int32_t *__restrict__ status) {
    extern __shared__ __align__(16) unsigned char lds[];
    int32_t *stage = reinterpret_cast<int32_t *>(lds);                               // [kLanes][kChunk + 1]
    uint16_t *lrow = reinterpret_cast<uint16_t *>(lds + kStage * sizeof(int32_t));  // [1 << kLutBits]
    int32_t *row = reinterpret_cast<int32_t *>(lds + kStage * sizeof(int32_t) + (sizeof(uint16_t) << kLutBits));
    const int lane = threadIdx.x;
    const int s0 = blockIdx.x * kLanes;
    const int s = s0 + lane;
    DevReader r{bytes, 0, 0, false, false, {}};
    bool active = false;
    uint64_t x = 0;
    if (s < n) {
        const int64_t a = offsets[s], b = offsets[s + 1];
        if (a < 0 || b < a || b > bytes_len) {
            status[s] = kStatusCorrupt;
        } else {
            r.p = a;
            r.end = b;
            r.aligned = ((reinterpret_cast<uintptr_t>(bytes) + (uintptr_t)a) & 3) == 0;
            r.start();
            x = r.next();
            x |= (uint64_t)r.next() << 32;
            active = !r.bad;
            status[s] = active ? CAE_OK : kStatusCorrupt;  // shorter than the 8-byte coder state
        }
    }
    const size_t per = (size_t)C * hw;
    const int nchunks = (hw + kChunk - 1) / kChunk;
    for (int c = 0; c < C; ++c) {
        const int32_t nlen = len[c], maxv = nlen - 2, o = off[c];
        __syncthreads();  // the previous channel's rows are no longer read
        for (int v = lane; v < nlen; v += kLanes) row[v] = cdf[(size_t)c * stride + v];
        for (int b = lane; b < (1 << kLutBits); b += kLanes) lrow[b] = lut[((size_t)c << kLutBits) + b];
        __syncthreads();
        for (int k = 0; k < nchunks; ++k) {
            const int base = k * kChunk;
            const int cnt = min(kChunk, hw - base);
            int32_t *mine = stage + lane * (kChunk + 1);
            for (int j = 0; active && j < cnt; ++j) {
                uint64_t xx = x;
                const uint32_t cum = (uint32_t)(xx & 0xFFFFu);
                // largest v with row[v] <= cum: start at the bucket's first symbol, scan forward
                int32_t v = lrow[cum >> (16 - kLutBits)];
                while (v < maxv && (uint32_t)row[v + 1] <= cum) ++v;
                const uint32_t start = (uint32_t)row[v], freq = (uint32_t)(row[v + 1] - row[v]);
                xx = (uint64_t)freq * (xx >> kPrecision) + (xx & 0xFFFFu) - start;
                if (xx < kRansL) xx = (xx << 32) | r.next();
                if (v == maxv) {
                    int32_t val = (int32_t)get_bits(xx, r);
                    int32_t nb = val;
                    // the host reads on while the digit is 15 and then rejects a count above 8: stopping at the first
                    // count above 8 gives the same verdict in a bounded number of steps
                    while (val == (int32_t)kMaxBypass && !r.bad && nb <= 8) {
                        val = (int32_t)get_bits(xx, r);
                        nb += val;
                    }
                    if (nb > 8) {
                        r.bad = true;
                        nb = 0;
                    }
                    uint32_t raw = 0;
                    for (int d = 0; d < nb && !r.bad; ++d) {
                        val = (int32_t)get_bits(xx, r);
                        raw |= (uint32_t)val << (d * kBypassBits);
                    }
                    v = (int32_t)(raw >> 1);
                    if (raw & 1)
                        v = -v - 1;
                    else
                        v = (int32_t)((uint32_t)v + (uint32_t)maxv);  // (wraps instead of overflowing on damaged input)
                }
                x = xx;
                mine[j] = (int32_t)((uint32_t)v + (uint32_t)o);
                if (r.bad) {
                    active = false;
                    status[s] = kStatusCorrupt;  // ran past the end of the stream
                }
            }
            __syncthreads();
            for (int rr = 0; rr < kLanes; ++rr) {
                const int sr = s0 + rr;
                if (sr < n && lane < cnt)
                    symbols[(size_t)sr * per + (size_t)c * hw + base + lane] = stage[rr * (kChunk + 1) + lane];
            }
            __syncthreads();
        }
    }
}

}  // namespace

// Device copy of the coder tables, uploaded into a FRESH buffer whenever cae_model_set_entropy changed them (version);
// the buffer it replaces is released only after the device has drained, so no kernel sees a table change halfway.
// (Allocation and upload happen on the first device-coder call after a table change only.)
int Model::ensure_ent_device() {
    if (ent_dev.buf && ent_dev.version == ent_version) return CAE_OK;
    const EntropyTables &T = ent;
    const size_t C = (size_t)T.channels, S = (size_t)T.stride;
    DevEntropy d;
    d.enc = 0;
    d.cdf = align_up(d.enc + C * S * sizeof(EncSym), 256);
    d.lut = align_up(d.cdf + C * S * sizeof(int32_t), 256);
    d.len = align_up(d.lut + (C << kLutBits) * sizeof(uint16_t), 256);
    d.off = align_up(d.len + C * sizeof(int32_t), 256);
    const size_t bytes = align_up(d.off + C * sizeof(int32_t), 256);
    std::vector<unsigned char> host(bytes, 0);
    memcpy(host.data() + d.enc, T.enc.data(), C * S * sizeof(EncSym));
    memcpy(host.data() + d.cdf, T.cdf.data(), C * S * sizeof(int32_t));
    memcpy(host.data() + d.lut, T.lut.data(), (C << kLutBits) * sizeof(uint16_t));
    memcpy(host.data() + d.len, T.len.data(), C * sizeof(int32_t));
    memcpy(host.data() + d.off, T.off.data(), C * sizeof(int32_t));
    CAE_TRY(d.buf.upload(host.data(), bytes));
    if (ent_dev.buf) HIP_TRY(hipDeviceSynchronize());  // coder kernels may still read the previous tables
    d.version = ent_version;
    ent_dev = std::move(d);  // (frees the previous buffer)
    return CAE_OK;
}

}  // namespace cae

using namespace cae;

// argument checks shared by the device coder entry points (before anything touches the device)
static int device_coder_args(Model *m, int n, int hw) {
    if (n <= 0 || hw <= 0) return fail(CAE_ERR_ARG, "bad shape (n=%d, hw=%d)", n, hw);
    if (n > kMaxStreams)
        return fail(CAE_ERR_ARG, "%d streams exceed the %d of one device coder call: split the batch", n, kMaxStreams);
    if (m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if ((int64_t)m->ent.channels * hw >= INT_MAX)
        return fail(CAE_ERR_ARG, "stream of %d x %d symbols too long", m->ent.channels, hw);
    if (m->ent.stride > kMaxStride)
        return fail(CAE_ERR_UNSUPPORTED, "CDF rows of %d entries exceed the device coder's %d", m->ent.stride, kMaxStride);
    return CAE_OK;
}

extern "C" {

int cae_rans_encode_workspace(cae_model_t *mm, int n, int hw, size_t *bytes) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !bytes) return fail(CAE_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(m->mu);
    CAE_TRY(device_coder_args(m, n, hw));
    const int C = m->ent.channels;
    *bytes = EncLayout(n, count_parts(C, hw)).words + (size_t)n * ((size_t)C * hw + 2) * sizeof(uint32_t);
    return CAE_OK;
}

int cae_rans_encode_device(cae_model_t *mm, const int32_t *symbols, int n, int hw, uint8_t *out, size_t out_capacity,
                           int64_t *offsets, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !symbols || !out || !offsets || !status || !workspace) return fail(CAE_ERR_ARG, "NULL argument");
    if (((uintptr_t)out | (uintptr_t)workspace) & 15) return fail(CAE_ERR_ARG, "out / workspace not 16-byte aligned");
    std::lock_guard<std::mutex> lk(m->mu);
    CAE_TRY(device_coder_args(m, n, hw));
    const int C = m->ent.channels, S = m->ent.stride;
    const int P = count_parts(C, hw);
    const EncLayout L(n, P);
    const size_t least = L.words + (size_t)n * 2 * sizeof(uint32_t);
    if (workspace_bytes < least)
        return fail(CAE_ERR_ARG, "workspace of %zu bytes too small (at least %zu)", workspace_bytes, least);
    CAE_TRY(m->ensure_ent_device());
    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    const DevEntropy &d = m->ent_dev;
    const unsigned char *tb = d.buf.get<unsigned char>();
    const EncSym *enc = (const EncSym *)(tb + d.enc);
    const int32_t *len = (const int32_t *)(tb + d.len), *off = (const int32_t *)(tb + d.off);
    int64_t *part_steps = (int64_t *)(ws + L.steps), *cap_off = (int64_t *)(ws + L.cap_off), *lens = (int64_t *)(ws + L.lens);
    int32_t *part_flags = (int32_t *)(ws + L.flags);
    uint32_t *words = (uint32_t *)(ws + L.words);
    const int64_t region_words = (int64_t)((workspace_bytes - L.words) / sizeof(uint32_t));

    hipLaunchKernelGGL(rans_count_kernel, dim3(P, n), dim3(kCountThreads), 0, st, symbols, len, off, C, hw, P, part_steps,
                       part_flags);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rans_capacity_kernel, dim3(1), dim3(kScanThreads), 0, st, part_steps, part_flags, n, P,
                       (int64_t)C * hw, region_words, cap_off, status);
    HIP_TRY(hipGetLastError());
    const int enc_lds = kStage * (int)sizeof(int32_t) + S * (int)sizeof(EncSym);
    CAE_TRY(ensure_lds((const void *)rans_encode_kernel, enc_lds));
    hipLaunchKernelGGL(rans_encode_kernel, dim3((n + kLanes - 1) / kLanes), dim3(kLanes), enc_lds, st, enc, len, off, S, C,
                       hw, n, symbols, cap_off, words, lens, status);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rans_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, lens, n, (int64_t)out_capacity, offsets,
                       status);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rans_compact_kernel, dim3(16, n), dim3(256), 0, st, words, cap_off, lens, offsets, status,
                       (uint32_t *)out);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_rans_decode_device(cae_model_t *mm, const uint8_t *bytes, size_t bytes_len, const int64_t *offsets, int n, int hw,
                           int32_t *symbols, int32_t *status, void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !bytes || !offsets || !symbols || !status) return fail(CAE_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(m->mu);
    CAE_TRY(device_coder_args(m, n, hw));
    const int C = m->ent.channels, S = m->ent.stride;
    CAE_TRY(m->ensure_ent_device());
    const DevEntropy &d = m->ent_dev;
    const unsigned char *tb = d.buf.get<unsigned char>();
    const int dec_lds = kStage * (int)sizeof(int32_t) + ((int)sizeof(uint16_t) << kLutBits) + S * (int)sizeof(int32_t);
    CAE_TRY(ensure_lds((const void *)rans_decode_kernel, dec_lds));
    hipLaunchKernelGGL(rans_decode_kernel, dim3((n + kLanes - 1) / kLanes), dim3(kLanes), dec_lds, (hipStream_t)stream,
                       (const int32_t *)(tb + d.cdf), (const uint16_t *)(tb + d.lut), (const int32_t *)(tb + d.len),
                       (const int32_t *)(tb + d.off), S, C, hw, n, (const unsigned char *)bytes, (int64_t)bytes_len,
                       offsets, symbols, status);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // extern "C"
