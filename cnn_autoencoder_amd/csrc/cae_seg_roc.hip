// cae_seg_roc_hist: the logit histograms behind a slide's ROC curve and AUC, and their launcher (include/cae_hip.h,
// "ROC histograms of a one-class head").
//
// First launch: a block takes a contiguous span of one image's counted pixels, keeps a private uint32 [2][2^bits]
// histogram in dynamic LDS (128 KiB at 14 bits: one block per CU), counts with LDS integer adds and stores the whole
// table as one partial [image][block][2][2^bits] in the workspace, work or not.  Loads as seg_predict_kernel: 16-byte
// logit loads and 4-byte target loads behind the image's first aligned address, the pixels in front of it and behind the
// last whole group one per lane (block 0 of the image).  Lanes of a wave that hit the first active lane's word add
// once, by their number: a slide's background puts most of a wave on one or two words, and 64 adds to one LDS word
// take 64 turns.  Second launch: the partials of an image, or of all images, summed into int64 in a fixed order
// (seg_histsum_kernel, cae_seg_merge.hip).  No global atomics, no float atomics, nothing to initialise.  The counted
// extent, the aligned head, the bits range and the grid policy: cae_seg_metrics.hpp.
#include "cae_seg_metrics.hpp"
#include "cae_seg_roc_key.hpp"

namespace cae {
namespace {

constexpr int kThreads = 1024;      // 16 waves: the one block a CU holds at 14 bits keeps its four SIMDs loading
constexpr size_t kSpanMin = 8192;   // pixels below which a block of its own only adds a partial

struct RocArgs {
    const float *logits;
    const uint8_t *target;
    const int32_t *extent;  // [n][2] or null
    uint32_t *partial;      // [n][bx][2][B]
    int h, w, bits, bx;
};

__global__ __launch_bounds__(kThreads) void roc_hist_kernel(RocArgs a) {
    extern __shared__ uint32_t hist[];  // [2][B]
    const int n = blockIdx.x / a.bx, x = blockIdx.x % a.bx, tid = threadIdx.x;
    const uint32_t B = 1u << a.bits;
    const int shift = 32 - a.bits;
    for (uint32_t i = tid; i < 2 * B; i += kThreads) hist[i] = 0;
    __syncthreads();

    const size_t w = (size_t)a.w, hw = (size_t)a.h * w;
    int rows, cols;
    extent_of(a.extent, n, a.h, a.w, rows, cols);
    const size_t lim = cols > 0 ? (size_t)rows * w : 0;  // whole rows beyond `rows` are never loaded
    const bool ragged = cols < a.w;                      // columns beyond `cols` are loaded and left out
    const float *lg = a.logits + (size_t)n * hw;
    const uint8_t *tg = a.target + (size_t)n * hw;

    // pixels [head, tail) in groups of four behind 16-byte aligned addresses; the (at most six) others one per lane
    const size_t head = std::min(lim, aligned_head(lg));
    const size_t groups = (lim - head) / 4;
    const size_t per_block = (groups + a.bx - 1) / a.bx;
    const size_t g0 = std::min(groups, (size_t)x * per_block), g1 = std::min(groups, g0 + per_block);
    const bool tg_vec = (reinterpret_cast<uintptr_t>(tg + head) & 3) == 0;
    constexpr size_t step = 4 * (size_t)kThreads;
    const size_t dcol = step % w;
    size_t col = ragged && g0 + tid < g1 ? (head + 4 * (g0 + tid)) % w : 0;  // column of the group's first pixel
    for (size_t g = g0 + tid; g < g1; g += kThreads) {
        const size_t p = head + 4 * g;  // p + 3 < head + 4 groups <= lim <= hw
        const float4 q = *reinterpret_cast<const float4 *>(lg + p);
        uint32_t t4;
        if (tg_vec)
            t4 = *reinterpret_cast<const uint32_t *>(tg + p);
        else
            t4 = (uint32_t)tg[p] | (uint32_t)tg[p + 1] << 8 | (uint32_t)tg[p + 2] << 16 | (uint32_t)tg[p + 3] << 24;
        const float v[4] = {q.x, q.y, q.z, q.w};
        size_t c = col;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = !ragged || c < (size_t)cols;
            hist_add(hist, on, (((t4 >> (8 * j)) & 255u) ? B : 0u) + roc_bin(v[j], shift));
            if (++c == w) c = 0;
        }
        col += dcol;
        if (col >= w) col -= w;
    }
    const size_t tail = head + 4 * groups, singles = head + (lim - tail);
    if (x == 0 && (size_t)tid < singles) {
        const size_t p = (size_t)tid < head ? (size_t)tid : tail + ((size_t)tid - head);  // < lim
        const bool on = !ragged || p % w < (size_t)cols;
        hist_add(hist, on, (tg[p] ? B : 0u) + roc_bin(lg[p], shift));
    }
    __syncthreads();

    // every (image, block) stores its whole table; 16 bytes per lane (2 B >= 512 words, the partials 16-byte aligned)
    uint4 *dst = reinterpret_cast<uint4 *>(a.partial + (size_t)blockIdx.x * 2 * B);
    const uint4 *src = reinterpret_cast<const uint4 *>(hist);
    for (uint32_t i = tid; i < B / 2; i += kThreads) dst[i] = src[i];
}

bool shape_ok(int n, int h, int w, int bits) { return n >= 1 && h >= 1 && w >= 1 && bits_ok(bits); }

// blocks per image: one per kSpanMin pixels
int blocks_per_image(int n, int h, int w, int bits) {
    return blocks_for(n, (size_t)h * (size_t)w, kSpanMin, hist_blocks_target(bits));
}

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" int cae_seg_roc_blocks(int n, int h, int w, int bits) {
    return shape_ok(n, h, w, bits) ? blocks_per_image(n, h, w, bits) : 0;
}

extern "C" size_t cae_seg_roc_workspace(int n, int h, int w, int bits) {
    if (!shape_ok(n, h, w, bits)) return 0;
    return (size_t)n * blocks_per_image(n, h, w, bits) * (sizeof(uint32_t) << (bits + 1));
}

extern "C" int cae_seg_roc_hist(const float *logits, const uint8_t *target, const int32_t *extent, int n, int h, int w,
                                int bits, int per_image, int64_t *hist, void *workspace, size_t workspace_bytes,
                                void *stream) {
    if (!bits_ok(bits)) return refuse_bits("cae_seg_roc_hist", bits);
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_seg_roc_hist: bad shape n=%d h=%d w=%d", n, h, w);
    if (n == 0) return CAE_OK;
    if (!logits || !target || !hist) return fail(CAE_ERR_ARG, "cae_seg_roc_hist: NULL logits, target or histogram");
    if (misaligned(logits, 3)) return fail(CAE_ERR_ARG, "cae_seg_roc_hist: logits not 4-byte aligned");
    const size_t need = cae_seg_roc_workspace(n, h, w, bits);
    if (!workspace || workspace_bytes < need)
        return fail(CAE_ERR_ARG, "cae_seg_roc_hist: workspace too small: %zu bytes needed", need);
    if (misaligned(workspace, 15) || misaligned(hist, 7))
        return fail(CAE_ERR_ARG, "cae_seg_roc_hist: workspace not 16-byte or histogram not 8-byte aligned");
    RocArgs a;
    a.logits = logits, a.target = target, a.extent = extent, a.partial = static_cast<uint32_t *>(workspace);
    a.h = h, a.w = w, a.bits = bits, a.bx = blocks_per_image(n, h, w, bits);
    // a block's words are 32 bits wide: its span stays below 2^32 pixels
    if (((size_t)h * (size_t)w + a.bx - 1) / a.bx >> 32)
        return fail(CAE_ERR_ARG, "cae_seg_roc_hist: %d images of %d x %d pixels are too many for one call", n, h, w);
    const int lds = (int)(sizeof(uint32_t) << (bits + 1));
    CAE_TRY(ensure_lds(reinterpret_cast<const void *>(roc_hist_kernel), lds));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(roc_hist_kernel, dim3((unsigned)((size_t)n * a.bx)), dim3(kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return launch_seg_histsum(a.partial, n, a.bx, per_image, bits, reinterpret_cast<long long *>(hist), st);
}
