// cae_tile_byte_hist: the exact byte histogram of every tile of a batch, and its launcher (include/cae_hip.h, "Byte
// histograms of tiles").  It is the look a sparse slide takes at every tile the tissue mask calls background: the
// squared error of a skipped tile against the fill value is a function of these 256 counts.
//
// First launch: a block takes a contiguous span of one tile's counted bytes, keeps a private uint32 [256] table in LDS,
// counts with LDS integer adds and stores the table as one partial [tile][block][256] in the workspace, work or not.
// The span is that of roc_hist_kernel with 16 elements per group (cae_seg_span.hpp): 16-byte loads behind the tile's
// first aligned address, the (at most 30) bytes in front of it and behind the last whole group one per lane (block 0 of
// the tile); the next group is in flight while the lane counts the one it holds.  The input this exists for is the worst
// case of an LDS histogram -- a background tile puts almost every byte on two or three values, and 64 adds to one LDS
// word take 64 turns -- so lanes combine before they add: a lane whose 16 bytes are one value adds 16 once, and in both
// kinds of add the lanes of a wave that hold the value of the first waiting lane add once, by their number, kLeads
// times over before the rest add on their own (hist_add, cae_seg_metrics.hpp).  Second
// launch: the partials of a tile summed into int64 in a fixed order (seg_histsum_kernel, cae_seg_merge.hip, as it
// stands: 256 words are the table of "7 bits").  No global atomics, nothing to initialise.
#include "cae_seg_metrics.hpp"

namespace cae {
namespace {

constexpr int kThreads = 256;          // one lane per bin when the table is cleared and stored
constexpr int kBins = 256;
constexpr size_t kSpanMin = 8192;      // bytes below which a block of its own only adds a partial: two turns of a block
constexpr int kBlocksCap = 2048;       // blocks of a launch at which more would only add partials: eight per CU, all its waves
constexpr int kLeads = 2;              // values a wave combines per add before its lanes add on their own
constexpr int kSumBits = 7;            // launch_seg_histsum sums tables of 2 << bits words

struct TileArgs {
    const uint8_t *tiles;
    const int32_t *extent;  // [n][2] or null
    uint32_t *partial;      // [n][bx][256]
    size_t rowbytes, hwc;   // w c and h w c
    int h, w, c, bx;
};

__global__ __launch_bounds__(kThreads) void tile_byte_hist_kernel(TileArgs a) {
    static_assert(kThreads == kBins, "one lane per bin");
    static_assert(kThreads >= 2 * (16 - 1), "a lane per single");
    __shared__ uint32_t hist[kBins];
    const int n = blockIdx.x / a.bx, x = blockIdx.x % a.bx, tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();

    int rows, cols;
    extent_of(a.extent, n, a.h, a.w, rows, cols);
    const size_t rowbytes = a.rowbytes, colbytes = (size_t)cols * a.c;
    const uint8_t *tl = a.tiles + (size_t)n * a.hwc;

    // bytes [head, tail) in groups of 16 behind 16-byte aligned addresses; the (at most 30) others one per lane
    const Span<16> s = span_of<16>(span_offset<16>(tl), rowbytes, (size_t)rows, colbytes, (size_t)a.bx, (size_t)x, kThreads);
    size_t g = s.g0 + tid;
    size_t col = s.first_col(tid);  // place in its row of the group's first byte
    uint4 q = make_uint4(0, 0, 0, 0);
    if (g < s.g1) q = *reinterpret_cast<const uint4 *>(tl + s.head + 16 * g);  // + 15 < head + 16 groups <= lim <= hwc
    while (g < s.g1) {
        const size_t next = g + kThreads;
        uint4 q_next = make_uint4(0, 0, 0, 0);
        if (next < s.g1) q_next = *reinterpret_cast<const uint4 *>(tl + s.head + 16 * next);
        const uint32_t word[4] = {q.x, q.y, q.z, q.w};
        const uint32_t v0 = q.x & 255u;
        // all 16 bytes counted and of one value: one add of 16
        const bool flat = q.x == v0 * 0x01010101u && q.y == q.x && q.z == q.x && q.w == q.x &&
                          (!s.ragged || col + 16 <= colbytes);
        hist_add<16, kLeads>(hist, flat, v0);
        if (!flat) {
            size_t c = col;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                hist_add<1, kLeads>(hist, s.on(c), (word[j / 4] >> (8 * (j % 4))) & 255u);
                if (++c == rowbytes) c = 0;
            }
        }
        s.turn(col);
        q = q_next;
        g = next;
    }
    if ((size_t)tid < s.singles) {
        const size_t p = s.single(tid);  // < lim
        hist_add<1, kLeads>(hist, s.on(p % rowbytes), tl[p]);
    }
    __syncthreads();
    a.partial[(size_t)blockIdx.x * kBins + tid] = hist[tid];  // every (tile, block) stores its whole table
}

bool shape_ok(int n, int h, int w, int c) { return n >= 1 && h >= 1 && w >= 1 && c >= 1 && c <= 4; }

size_t tile_bytes(int h, int w, int c) { return (size_t)h * (size_t)w * (size_t)c; }  // < 2^64: h, w < 2^31, c <= 4

// blocks per tile: one per kSpanMin bytes
int blocks_per_tile(int n, int h, int w, int c) { return blocks_for(n, tile_bytes(h, w, c), kSpanMin, kBlocksCap); }

// a block's words are 32 bits wide: its span stays below 2^32 bytes
bool span_fits(int n, int h, int w, int c) {
    const size_t bx = (size_t)blocks_per_tile(n, h, w, c);
    return ((tile_bytes(h, w, c) + bx - 1) / bx + 32) >> 32 == 0;
}

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" int cae_tile_byte_hist_blocks(int n, int h, int w, int c) {
    return shape_ok(n, h, w, c) && span_fits(n, h, w, c) ? blocks_per_tile(n, h, w, c) : 0;
}

extern "C" size_t cae_tile_byte_hist_workspace(int n, int h, int w, int c) {
    return (size_t)std::max(n, 0) * (size_t)cae_tile_byte_hist_blocks(n, h, w, c) * kBins * sizeof(uint32_t);
}

extern "C" int cae_tile_byte_hist(const uint8_t *tiles, const int32_t *extent, int n, int h, int w, int c, int64_t *hist,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_tile_byte_hist: bad shape n=%d h=%d w=%d", n, h, w);
    if (c < 1 || c > 4) return fail(CAE_ERR_ARG, "cae_tile_byte_hist: %d channels outside 1..4", c);
    if (!span_fits(std::max(n, 1), h, w, c))
        return fail(CAE_ERR_ARG, "cae_tile_byte_hist: tiles of %d x %d x %d bytes are too large for the spans of one call", h, w, c);
    if (n == 0) return CAE_OK;
    if (!tiles || !hist) return fail(CAE_ERR_ARG, "cae_tile_byte_hist: NULL tiles or histogram");
    if (misaligned(extent, 3) || misaligned(hist, 7))
        return fail(CAE_ERR_ARG, "cae_tile_byte_hist: extent not 4-byte or histogram not 8-byte aligned");
    const size_t need = cae_tile_byte_hist_workspace(n, h, w, c);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 15))
        return fail(CAE_ERR_ARG, "cae_tile_byte_hist: workspace NULL, not 16-byte aligned or too small: %zu bytes needed", need);
    TileArgs a;
    a.tiles = tiles, a.extent = extent, a.partial = static_cast<uint32_t *>(workspace);
    a.rowbytes = (size_t)w * c, a.hwc = tile_bytes(h, w, c);
    a.h = h, a.w = w, a.c = c, a.bx = blocks_per_tile(n, h, w, c);
    if ((size_t)n * a.bx > (size_t)INT_MAX) return fail(CAE_ERR_ARG, "cae_tile_byte_hist: %d tiles are too many for one call", n);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tile_byte_hist_kernel, dim3((unsigned)((size_t)n * a.bx)), dim3(kThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return launch_seg_histsum(a.partial, n, a.bx, 1, kSumBits, reinterpret_cast<long long *>(hist), st);
}
