// cae_seg_roc_hist and cae_seg_score_hist: the logit histograms behind a slide's ROC curve and AUC, the score histograms
// behind its average precision, and their launcher (include/cae_hip.h, "ROC histograms of a one-class head" and "Score
// histograms of a head of several classes").  One walk; a policy says what the two differ in: which plane of values a
// block reads (an image's one plane of logits, or one class plane of an image's scores), which labels count, which are
// positive, and the bin of a value.
//
// First launch: a block takes a contiguous span of one plane's counted pixels (cae_seg_span.hpp), keeps a private uint32
// [2][2^bits] histogram in dynamic LDS (128 KiB at 14 bits: one block per CU), counts with LDS integer adds (hist_add) and
// stores the whole table as one partial per (plane, block) in the workspace, work or not.  Loads as seg_predict_kernel:
// 16-byte value loads and 4-byte target loads behind the plane's first aligned address, the pixels in front of it and
// behind the last whole group one per lane (block 0 of the plane); class planes of h w pixels that are no multiple of
// four start at every alignment.  Every class plane reads its image's target again: C bytes per pixel beside the 4 C of
// the scores.  Second launch: the partials of an output summed into int64 in a fixed order (seg_histsum_kernel,
// cae_seg_merge.hip); the partials of the scores lie image-major, or class-major where classes are kept apart and images
// are not, so that those of one output are neighbours.  No global atomics, no float atomics, nothing to initialise.  The
// counted extent, the bits range and the grid policy: cae_seg_metrics.hpp; the bins: cae_seg_roc_key.hpp,
// cae_seg_score_bin.hpp.
#include "cae_seg_metrics.hpp"
#include "cae_seg_roc_key.hpp"
#include "cae_seg_score_bin.hpp"

namespace cae {
namespace {

constexpr int kThreads = 1024;      // 16 waves: the one block a CU holds at 14 bits keeps its four SIMDs loading
constexpr size_t kSpanMin = 8192;   // pixels below which a block of its own only adds a partial
constexpr int kMinClasses = 2, kMaxClasses = 255;  // a label is a byte, and 255 marks the padding of a slide's edge tiles

struct HistArgs {
    const float *values;    // logits [n][h][w], or scores [n][c][h][w]
    const uint8_t *target;  // [n][h][w]
    const int32_t *extent;  // [n][2] or null
    uint32_t *partial;      // [n][bx][2][B]; scores: [n][c][bx][2][B], or [c][n][bx][2][B] with class_major
    int n, c, h, w, bits, bx, class_major;
};

// plane = image; every label counts, and any but 0 is positive
struct RocPolicy {
    int image, plane, shift;
    __device__ RocPolicy(const HistArgs &a, int p) : image(p), plane(p), shift(32 - a.bits) {}
    __device__ bool counted(uint32_t) const { return true; }
    __device__ bool positive(uint32_t t) const { return t != 0; }
    __device__ uint32_t bin(float v) const { return roc_bin(v, shift); }
};

// plane = (image, class k); a label outside the classes is in no histogram, and k is the positive one
struct ScorePolicy {
    const HistArgs &a;
    int image, plane;
    uint32_t K;
    __device__ ScorePolicy(const HistArgs &args, int p) : a(args) {
        image = a.class_major ? p % a.n : p / a.c;
        K = (uint32_t)(a.class_major ? p / a.n : p % a.c);
        plane = image * a.c + (int)K;  // < n c <= INT_MAX
    }
    __device__ bool counted(uint32_t t) const { return t < (uint32_t)a.c; }
    __device__ bool positive(uint32_t t) const { return t == K; }
    __device__ uint32_t bin(float v) const { return score_bin(v, a.bits); }
};

__device__ __forceinline__ void table_clear(uint32_t *hist, uint32_t words) {
    for (uint32_t i = threadIdx.x; i < words; i += kThreads) hist[i] = 0;
    __syncthreads();
}

// 16 bytes per lane (`words` >= 512, a multiple of four; dst 16-byte aligned)
__device__ __forceinline__ void table_store(const uint32_t *hist, uint32_t words, uint32_t *dst) {
    __syncthreads();
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint4 *s = reinterpret_cast<const uint4 *>(hist);
    for (uint32_t i = threadIdx.x; i < words / 4; i += kThreads) d[i] = s[i];
}

template <typename Policy>
__device__ __forceinline__ void value_hist(const HistArgs &a) {
    static_assert(kThreads >= 2 * (4 - 1), "a lane per single");
    extern __shared__ uint32_t hist[];  // [2][B]
    const int x = blockIdx.x % a.bx, tid = threadIdx.x;
    const Policy pl(a, blockIdx.x / a.bx);
    const uint32_t B = 1u << a.bits;
    table_clear(hist, 2 * B);

    const size_t w = (size_t)a.w, hw = (size_t)a.h * w;
    int rows, cols;
    extent_of(a.extent, pl.image, a.h, a.w, rows, cols);
    const float *val = a.values + (size_t)pl.plane * hw;
    const uint8_t *tg = a.target + (size_t)pl.image * hw;

    // pixels [head, tail) in groups of four behind 16-byte aligned addresses; the (at most six) others one per lane
    const Span<4> s = span_of<4>(span_offset<4>(val), w, (size_t)rows, (size_t)cols, (size_t)a.bx, (size_t)x, kThreads);
    const bool tg_vec = (reinterpret_cast<uintptr_t>(tg + s.head) & 3) == 0;
    size_t col = s.first_col(tid);  // column of the group's first pixel
    for (size_t g = s.g0 + tid; g < s.g1; g += kThreads) {
        const size_t p = s.head + 4 * g;  // p + 3 < head + 4 groups <= lim <= hw
        const float4 q = *reinterpret_cast<const float4 *>(val + p);
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
            hist_add<1, 1>(hist, pl.counted(t) && s.on(c), (pl.positive(t) ? B : 0u) + pl.bin(v[j]));
            if (++c == w) c = 0;
        }
        s.turn(col);
    }
    if ((size_t)tid < s.singles) {
        const size_t p = s.single(tid);  // < lim
        const uint32_t t = tg[p];
        hist_add<1, 1>(hist, pl.counted(t) && s.on(p % w), (pl.positive(t) ? B : 0u) + pl.bin(val[p]));
    }
    // every (plane, block) stores its whole table
    table_store(hist, 2 * B, a.partial + (size_t)blockIdx.x * 2 * B);
}

__global__ __launch_bounds__(kThreads) void roc_hist_kernel(HistArgs a) { value_hist<RocPolicy>(a); }
__global__ __launch_bounds__(kThreads) void score_hist_kernel(HistArgs a) { value_hist<ScorePolicy>(a); }

// blocks per plane: one per kSpanMin pixels
int blocks_per_plane(int planes, int h, int w, int bits) {
    return blocks_for(planes, (size_t)h * (size_t)w, kSpanMin, hist_blocks_target(bits));
}

size_t table_bytes(int bits) { return sizeof(uint32_t) << (bits + 1); }

bool roc_shape_ok(int n, int h, int w, int bits) { return n >= 1 && h >= 1 && w >= 1 && bits_ok(bits); }

// a plane holds at most INT_MAX pixels: a block's span, and so each of its 32-bit words, stays below 2^31
bool score_shape_ok(int n, int c, int h, int w, int bits) {
    return n >= 1 && c >= kMinClasses && c <= kMaxClasses && h >= 1 && w >= 1 && (long long)h * w <= INT_MAX &&
           (long long)n * c <= INT_MAX && bits_ok(bits);
}

// What both entry points do behind their own shape rules: the pointer and workspace checks, the LDS opt-in, the launch
// over n c planes and the merge into `outputs` histograms, whose partials are neighbours.  `what`: the values' name
int launch_value_hist(const char *who, const char *what, void (*kernel)(HistArgs), HistArgs a, int outputs, int64_t *hist,
                      void *workspace, size_t workspace_bytes, void *stream) {
    if (!a.values || !a.target || !hist) return fail(CAE_ERR_ARG, "%s: NULL %s, target or histogram", who, what);
    if (misaligned(a.values, 3)) return fail(CAE_ERR_ARG, "%s: %s not 4-byte aligned", who, what);
    a.bx = blocks_per_plane(a.n * a.c, a.h, a.w, a.bits);
    const size_t blocks = (size_t)a.n * a.c * a.bx;  // <= max(n c, the cap of hist_blocks_target): inside a grid
    const size_t need = blocks * table_bytes(a.bits);
    if (!workspace || workspace_bytes < need) return fail(CAE_ERR_ARG, "%s: workspace too small: %zu bytes needed", who, need);
    if (misaligned(workspace, 15) || misaligned(hist, 7))
        return fail(CAE_ERR_ARG, "%s: workspace not 16-byte or histogram not 8-byte aligned", who);
    a.partial = static_cast<uint32_t *>(workspace);
    const int lds = (int)table_bytes(a.bits);
    CAE_TRY(ensure_lds(reinterpret_cast<const void *>(kernel), lds));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return launch_seg_histsum(a.partial, outputs, (int)(blocks / outputs), 1, a.bits, reinterpret_cast<long long *>(hist), st);
}

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" int cae_seg_roc_blocks(int n, int h, int w, int bits) {
    return roc_shape_ok(n, h, w, bits) ? blocks_per_plane(n, h, w, bits) : 0;
}

extern "C" size_t cae_seg_roc_workspace(int n, int h, int w, int bits) {
    if (!roc_shape_ok(n, h, w, bits)) return 0;
    return (size_t)n * blocks_per_plane(n, h, w, bits) * table_bytes(bits);
}

extern "C" int cae_seg_roc_hist(const float *logits, const uint8_t *target, const int32_t *extent, int n, int h, int w,
                                int bits, int per_image, int64_t *hist, void *workspace, size_t workspace_bytes,
                                void *stream) {
    const char *who = "cae_seg_roc_hist";
    if (!bits_ok(bits)) return refuse_bits(who, bits);
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    if (n == 0) return CAE_OK;
    // a block's words are 32 bits wide: its span stays below 2^32 pixels
    const size_t bx = (size_t)blocks_per_plane(n, h, w, bits);
    if (((size_t)h * (size_t)w + bx - 1) / bx >> 32)
        return fail(CAE_ERR_ARG, "%s: %d images of %d x %d pixels are too many for one call", who, n, h, w);
    HistArgs a = {logits, target, extent, nullptr, n, 1, h, w, bits, 0, 0};
    return launch_value_hist(who, "logits", roc_hist_kernel, a, per_image ? n : 1, hist, workspace, workspace_bytes, stream);
}

extern "C" size_t cae_seg_score_workspace(int n, int c, int h, int w, int bits) {
    if (!score_shape_ok(n, c, h, w, bits)) return 0;
    return (size_t)n * c * blocks_per_plane(n * c, h, w, bits) * table_bytes(bits);
}

extern "C" int cae_seg_score_hist(const float *scores, const uint8_t *target, const int32_t *extent, int n, int c, int h,
                                  int w, int bits, int per_image, int per_class, int64_t *hist, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    const char *who = "cae_seg_score_hist";
    if (!bits_ok(bits)) return refuse_bits(who, bits);
    if (c < kMinClasses || c > kMaxClasses)
        return fail(CAE_ERR_ARG, "%s: %d classes outside %d..%d", who, c, kMinClasses, kMaxClasses);
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    if (!score_shape_ok(n, c, h, w, bits))
        return fail(CAE_ERR_ARG, "%s: %d x %d planes of %d x %d pixels are too large", who, n, c, h, w);
    HistArgs a = {scores, target, extent, nullptr, n, c, h, w, bits, 0, per_class && !per_image};
    // outputs [n or 1][c or 1]: the partials of each are neighbours in the order chosen above
    return launch_value_hist(who, "scores", score_hist_kernel, a, (per_image ? n : 1) * (per_class ? c : 1), hist, workspace,
                             workspace_bytes, stream);
}
