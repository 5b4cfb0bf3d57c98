// cae_seg_score_hist: the score histograms behind a slide's average precision, and their launcher (include/cae_hip.h,
// "Score histograms of a head of several classes").  The sibling of cae_seg_roc_hist (cae_seg_roc.hip) with one class
// plane where that has one image.
//
// First launch: a block takes a contiguous span of one class plane's counted pixels, keeps a private uint32 [2][2^bits]
// histogram in dynamic LDS (128 KiB at 14 bits: one block per CU), counts with LDS integer adds (hist_add) and stores the
// whole table as one partial per (plane, block) in the workspace, work or not.  Loads as roc_hist_kernel: 16-byte score
// loads and 4-byte target loads behind the plane's first aligned address, the pixels in front of it and behind the last
// whole group one per lane (block 0 of the plane); planes of h w pixels that are no multiple of four start at every
// alignment.  Every plane reads its image's target again: C bytes per pixel beside the 4 C of the scores.  Second launch:
// the partials of an output summed into int64 in a fixed order (seg_histsum_kernel, cae_seg_merge.hip); the partials lie
// image-major, or class-major where classes are kept apart and images are not, so that those of one output are
// neighbours.  No global atomics, no float atomics, nothing to initialise.  The counted extent, the aligned head, the bits
// range and the grid policy: cae_seg_metrics.hpp; the bin: cae_seg_score_bin.hpp.
#include "cae_seg_metrics.hpp"
#include "cae_seg_score_bin.hpp"

namespace cae {
namespace {

constexpr int kThreads = 1024;      // 16 waves: the one block a CU holds at 14 bits keeps its four SIMDs loading
constexpr size_t kSpanMin = 8192;   // pixels below which a block of its own only adds a partial
constexpr int kMinClasses = 2, kMaxClasses = 255;  // a label is a byte, and 255 marks the padding of a slide's edge tiles

struct ScoreArgs {
    const float *scores;    // [n][c][h][w]
    const uint8_t *target;  // [n][h][w]
    const int32_t *extent;  // [n][2] or null
    uint32_t *partial;      // [n][c][bx][2][B], or [c][n][bx][2][B] with class_major
    int n, c, h, w, bits, bx, class_major;
};

__global__ __launch_bounds__(kThreads) void score_hist_kernel(ScoreArgs a) {
    extern __shared__ uint32_t hist[];  // [2][B]
    const int x = blockIdx.x % a.bx, plane = blockIdx.x / a.bx, tid = threadIdx.x;
    const int n = a.class_major ? plane % a.n : plane / a.c, k = a.class_major ? plane / a.n : plane % a.c;
    const uint32_t B = 1u << a.bits, C = (uint32_t)a.c, K = (uint32_t)k;
    for (uint32_t i = tid; i < 2 * B; i += kThreads) hist[i] = 0;
    __syncthreads();

    const size_t w = (size_t)a.w, hw = (size_t)a.h * w;
    int rows, cols;
    extent_of(a.extent, n, a.h, a.w, rows, cols);
    const size_t lim = cols > 0 ? (size_t)rows * w : 0;  // whole rows beyond `rows` are never loaded
    const bool ragged = cols < a.w;                      // columns beyond `cols` are loaded and left out
    const float *sc = a.scores + ((size_t)n * a.c + k) * hw;
    const uint8_t *tg = a.target + (size_t)n * hw;

    // pixels [head, tail) in groups of four behind 16-byte aligned addresses; the (at most six) others one per lane
    const size_t head = std::min(lim, aligned_head(sc));
    const size_t groups = (lim - head) / 4;
    const size_t per_block = (groups + a.bx - 1) / a.bx;
    const size_t g0 = std::min(groups, (size_t)x * per_block), g1 = std::min(groups, g0 + per_block);
    const bool tg_vec = (reinterpret_cast<uintptr_t>(tg + head) & 3) == 0;
    constexpr size_t step = 4 * (size_t)kThreads;
    const size_t dcol = step % w;
    size_t col = ragged && g0 + tid < g1 ? (head + 4 * (g0 + tid)) % w : 0;  // column of the group's first pixel
    for (size_t g = g0 + tid; g < g1; g += kThreads) {
        const size_t p = head + 4 * g;  // p + 3 < head + 4 groups <= lim <= hw
        const float4 q = *reinterpret_cast<const float4 *>(sc + p);
        uint32_t t4;
        if (tg_vec)
            t4 = *reinterpret_cast<const uint32_t *>(tg + p);
        else
            t4 = (uint32_t)tg[p] | (uint32_t)tg[p + 1] << 8 | (uint32_t)tg[p + 2] << 16 | (uint32_t)tg[p + 3] << 24;
        const float v[4] = {q.x, q.y, q.z, q.w};
        size_t c = col;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t t = (t4 >> (8 * j)) & 255u;
            const bool on = t < C && (!ragged || c < (size_t)cols);  // a label outside the classes is in no histogram
            hist_add(hist, on, (t == K ? B : 0u) + score_bin(v[j], a.bits));
            if (++c == w) c = 0;
        }
        col += dcol;
        if (col >= w) col -= w;
    }
    const size_t tail = head + 4 * groups, singles = head + (lim - tail);
    if (x == 0 && (size_t)tid < singles) {
        const size_t p = (size_t)tid < head ? (size_t)tid : tail + ((size_t)tid - head);  // < lim
        const uint32_t t = tg[p];
        const bool on = t < C && (!ragged || p % w < (size_t)cols);
        hist_add(hist, on, (t == K ? B : 0u) + score_bin(sc[p], a.bits));
    }
    __syncthreads();

    // every (plane, block) stores its whole table; 16 bytes per lane (2 B >= 512 words, the partials 16-byte aligned)
    uint4 *dst = reinterpret_cast<uint4 *>(a.partial + (size_t)blockIdx.x * 2 * B);
    const uint4 *src = reinterpret_cast<const uint4 *>(hist);
    for (uint32_t i = tid; i < B / 2; i += kThreads) dst[i] = src[i];
}

// a plane holds at most INT_MAX pixels: a block's span, and so each of its 32-bit words, stays below 2^31
bool shape_ok(int n, int c, int h, int w, int bits) {
    return n >= 1 && c >= kMinClasses && c <= kMaxClasses && h >= 1 && w >= 1 && (long long)h * w <= INT_MAX &&
           (long long)n * c <= INT_MAX && bits_ok(bits);
}

// blocks per class plane: one per kSpanMin pixels
int blocks_per_plane(int n, int c, int h, int w, int bits) {
    return blocks_for(n * c, (size_t)h * (size_t)w, kSpanMin, hist_blocks_target(bits));
}

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" size_t cae_seg_score_workspace(int n, int c, int h, int w, int bits) {
    if (!shape_ok(n, c, h, w, bits)) return 0;
    return (size_t)n * c * blocks_per_plane(n, c, h, w, bits) * (sizeof(uint32_t) << (bits + 1));
}

extern "C" int cae_seg_score_hist(const float *scores, const uint8_t *target, const int32_t *extent, int n, int c, int h,
                                  int w, int bits, int per_image, int per_class, int64_t *hist, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!bits_ok(bits)) return refuse_bits("cae_seg_score_hist", bits);
    if (c < kMinClasses || c > kMaxClasses)
        return fail(CAE_ERR_ARG, "cae_seg_score_hist: %d classes outside %d..%d", c, kMinClasses, kMaxClasses);
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_seg_score_hist: bad shape n=%d h=%d w=%d", n, h, w);
    if (!shape_ok(n, c, h, w, bits))
        return fail(CAE_ERR_ARG, "cae_seg_score_hist: %d x %d planes of %d x %d pixels are too large", n, c, h, w);
    if (!scores || !target || !hist) return fail(CAE_ERR_ARG, "cae_seg_score_hist: NULL scores, target or histogram");
    if (misaligned(scores, 3)) return fail(CAE_ERR_ARG, "cae_seg_score_hist: scores not 4-byte aligned");
    const size_t need = cae_seg_score_workspace(n, c, h, w, bits);
    if (!workspace || workspace_bytes < need)
        return fail(CAE_ERR_ARG, "cae_seg_score_hist: workspace too small: %zu bytes needed", need);
    if (misaligned(workspace, 15) || misaligned(hist, 7))
        return fail(CAE_ERR_ARG, "cae_seg_score_hist: workspace not 16-byte or histogram not 8-byte aligned");
    ScoreArgs a;
    a.scores = scores, a.target = target, a.extent = extent, a.partial = static_cast<uint32_t *>(workspace);
    a.n = n, a.c = c, a.h = h, a.w = w, a.bits = bits, a.bx = blocks_per_plane(n, c, h, w, bits);
    a.class_major = per_class && !per_image;
    const size_t blocks = (size_t)n * c * a.bx;  // <= max(n c, the cap of hist_blocks_target): inside a grid
    const int lds = (int)(sizeof(uint32_t) << (bits + 1));
    CAE_TRY(ensure_lds(reinterpret_cast<const void *>(score_hist_kernel), lds));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(score_hist_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    // outputs [n or 1][c or 1]: the partials of each are neighbours in the order chosen above
    const int outputs = (per_image ? n : 1) * (per_class ? c : 1);
    return launch_seg_histsum(a.partial, outputs, (int)(blocks / outputs), 1, bits, reinterpret_cast<long long *>(hist), st);
}
