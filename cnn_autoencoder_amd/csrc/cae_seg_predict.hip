// cae_seg_predict: the segmentation head's logits -> class map, scores and confusion counts in one pass, and its
// launcher (include/cae_hip.h, "Prediction from the head's logits").
//
// One block walks groups of four consecutive pixels of one image: a lane loads the four pixels of every class plane with
// one 16-byte access, decides, and stores the class bytes with one 4-byte and the scores with 16-byte accesses.  The
// 16-byte path needs every plane of the image to start at the same offset within 16 bytes, i.e. one class or HW a
// multiple of four; the pixels in front of the first aligned address and behind the last whole group (at most three
// each) -- and every pixel otherwise -- go one pixel per lane.  Up to kRegC classes the logits of a pixel live in
// registers and are read from HBM once; above it the planes are streamed three times (maximum, sum, scores), the second
// and third time out of the cache.  Counts are integers: lane tallies, summed over the wave by shuffles, over the block
// through LDS, one partial per (image, block) in the workspace, merged by seg_record_kernel; no atomics, exact.  The
// decisions of one class and of streamed planes, the block tally, the grid policy and the merge: cae_seg_metrics.hpp.
#include "cae_seg_metrics.hpp"

namespace cae {
namespace {

constexpr int kThreads = 256;
constexpr int kRegC = 16;  // classes held in registers (four pixels each: 64 VGPRs of logits)

struct PredictArgs {
    const float *logits;
    const uint8_t *target;
    uint8_t *cls;
    float *scores;
    unsigned long long *partial;  // [n][bx][kPartial] or null
    size_t hw;
    int c, top_k, bx;
    float t;
};

// l[0..C): the pixel's logits, overwritten by its scores if `want`.  -> class index
template <int CMAX>
__device__ __forceinline__ uint8_t decide_multi(float (&l)[CMAX], int C, int tgt, int k, bool want, Tally<unsigned> &ty) {
    float best = l[0];
    int idx = 0;
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C && above(l[c], best)) {  // strict: idx stays in 0..C-1
            best = l[c];
            idx = c;
        }
    if (tgt >= 0) {
        ty.v[0] += idx == tgt;
        float lt = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) lt = c == tgt ? l[c] : lt;
        int rank = 0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) rank += c < C && before(l[c], c, lt, tgt);
        ty.v[1] += tgt < C && rank < k;
    }
    if (want) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                l[c] = __expf(l[c] - best);  // argument <= 0
                s += l[c];
            }
        const float r = 1.0f / s;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) l[c] *= r;
    }
    return (uint8_t)idx;
}

template <int CMAX>
__device__ __forceinline__ uint8_t decide_pixel(float (&l)[CMAX], const PredictArgs &a, int tgt, bool want,
                                                Tally<unsigned> &ty) {
    if constexpr (CMAX == 1)
        return decide_binary(l[0], a.t, tgt, want, 1u, ty);
    else
        return decide_multi<CMAX>(l, a.c, tgt, a.top_k, want, ty);
}

// CMAX: 1 = one class (threshold), 2 / 4 / 8 / 16 = up to that many classes in registers, 0 = streamed
template <int CMAX>
__global__ __launch_bounds__(kThreads) void seg_predict_kernel(PredictArgs a) {
    const int n = blockIdx.x / a.bx, x = blockIdx.x % a.bx, tid = threadIdx.x;
    const size_t hw = a.hw;
    const int C = a.c;
    const float *lg = a.logits + (size_t)n * C * hw;
    float *sc = a.scores ? a.scores + (size_t)n * C * hw : nullptr;
    const uint8_t *tg = a.target ? a.target + (size_t)n * hw : nullptr;
    uint8_t *cl = a.cls + (size_t)n * hw;
    const size_t stride = (size_t)a.bx * kThreads, first = (size_t)x * kThreads + tid;
    Tally<unsigned> ty = {{0, 0, 0, 0}};

    // pixels [head, tail) in groups of four behind 16-byte aligned addresses; the rest one by one
    size_t head = hw, groups = 0;
    if constexpr (CMAX != 0) {
        constexpr int R = CMAX;
        if (C == 1 || hw % 4 == 0) {
            head = std::min(hw, aligned_head(lg));
            groups = (hw - head) / 4;
        }
        // scores share the 16-byte path if they sit at the logits' offset within 16 bytes; class and target bytes go
        // four at a time from 4-byte aligned addresses
        const bool sc_vec = sc && ((reinterpret_cast<uintptr_t>(sc) ^ reinterpret_cast<uintptr_t>(lg)) & 15) == 0;
        const bool cl_vec = (reinterpret_cast<uintptr_t>(cl + head) & 3) == 0;
        const bool tg_vec = tg && (reinterpret_cast<uintptr_t>(tg + head) & 3) == 0;
        for (size_t g = first; g < groups; g += stride) {
            const size_t p = head + 4 * g;  // p + 3 < head + 4 groups <= hw
            float v[R][4];
#pragma unroll
            for (int c = 0; c < R; ++c) {
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < C) q = *reinterpret_cast<const float4 *>(lg + (size_t)c * hw + p);
                v[c][0] = q.x, v[c][1] = q.y, v[c][2] = q.z, v[c][3] = q.w;
            }
            int t4[4] = {-1, -1, -1, -1};
            if (tg) {
                if (tg_vec) {
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(tg + p);
#pragma unroll
                    for (int j = 0; j < 4; ++j) t4[j] = (w >> (8 * j)) & 255;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) t4[j] = tg[p + j];
                }
            }
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float l[R];
#pragma unroll
                for (int c = 0; c < R; ++c) l[c] = v[c][j];
                packed |= (uint32_t)decide_pixel<R>(l, a, t4[j], sc != nullptr, ty) << (8 * j);
#pragma unroll
                for (int c = 0; c < R; ++c) v[c][j] = l[c];
            }
            if (cl_vec) {
                *reinterpret_cast<uint32_t *>(cl + p) = packed;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) cl[p + j] = (uint8_t)(packed >> (8 * j));
            }
            if (sc) {
#pragma unroll
                for (int c = 0; c < R; ++c)
                    if (c < C) {
                        float *dst = sc + (size_t)c * hw + p;
                        if (sc_vec) {
                            *reinterpret_cast<float4 *>(dst) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j) dst[j] = v[c][j];
                        }
                    }
            }
        }
    }
    const size_t tail = head + 4 * groups, singles = head + (hw - tail);
    for (size_t q = first; q < singles; q += stride) {
        const size_t p = q < head ? q : tail + (q - head);  // < hw
        const int tgt = tg ? (int)tg[p] : -1;
        if constexpr (CMAX == 0) {
            cl[p] = sc ? decide_stream<true>(lg, sc, hw, p, C, tgt, a.top_k, 1u, ty)
                       : decide_stream<false>(lg, sc, hw, p, C, tgt, a.top_k, 1u, ty);
        } else {
            constexpr int R = CMAX;
            float l[R];
#pragma unroll
            for (int c = 0; c < R; ++c) l[c] = c < C ? lg[(size_t)c * hw + p] : 0.f;
            cl[p] = decide_pixel<R>(l, a, tgt, sc != nullptr, ty);
            if (sc) {
#pragma unroll
                for (int c = 0; c < R; ++c)
                    if (c < C) sc[(size_t)c * hw + p] = l[c];
            }
        }
    }

    if (a.partial) block_tally_store<kThreads>(ty, a.partial);
}

// blocks per image: one per 256 groups of four pixels
int blocks_per_image(int n, size_t hw) { return blocks_for(n, hw, 4 * kThreads, kBlocksTarget); }

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" size_t cae_seg_predict_workspace(int n, int c, size_t hw) {
    if (n < 1 || c < 1 || c > 256 || hw < 1) return 0;
    return (size_t)n * blocks_per_image(n, hw) * kPartial * sizeof(unsigned long long);
}

extern "C" int cae_seg_predict(const float *logits, const uint8_t *target, int n, int c, size_t hw, float t, int top_k,
                               uint8_t *cls, float *scores, int64_t *counts, void *workspace, size_t workspace_bytes,
                               void *stream) {
    if (c < 1 || c > 256) return fail(CAE_ERR_ARG, "cae_seg_predict: %d classes outside 1..256", c);
    if (n < 0 || hw < 1) return fail(CAE_ERR_ARG, "cae_seg_predict: bad shape n=%d hw=%zu", n, hw);
    if (top_k < 1) return fail(CAE_ERR_ARG, "cae_seg_predict: top_k %d below 1", top_k);
    if (counts && !target) return fail(CAE_ERR_ARG, "cae_seg_predict: counts need a target");
    if (n == 0) return CAE_OK;
    if (!logits || !cls) return fail(CAE_ERR_ARG, "cae_seg_predict: NULL logits or class map");
    const size_t need = cae_seg_predict_workspace(n, c, hw);
    if (counts && (!workspace || workspace_bytes < need))
        return fail(CAE_ERR_ARG, "cae_seg_predict: workspace too small: %zu bytes needed", need);
    if (counts && misaligned(workspace, 7))
        return fail(CAE_ERR_ARG, "cae_seg_predict: workspace not 8-byte aligned");
    PredictArgs a;
    a.logits = logits, a.target = target, a.cls = cls, a.scores = scores;
    a.partial = counts ? static_cast<unsigned long long *>(workspace) : nullptr;
    a.hw = hw, a.c = c, a.top_k = std::min(top_k, c), a.bx = blocks_per_image(n, hw), a.t = t;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((size_t)n * a.bx)), block(kThreads);  // n bx <= max(n, kBlocksTarget)
    if (c == 1)
        hipLaunchKernelGGL(seg_predict_kernel<1>, grid, block, 0, st, a);
    else if (c <= 2)
        hipLaunchKernelGGL(seg_predict_kernel<2>, grid, block, 0, st, a);
    else if (c <= 4)
        hipLaunchKernelGGL(seg_predict_kernel<4>, grid, block, 0, st, a);
    else if (c <= 8)
        hipLaunchKernelGGL(seg_predict_kernel<8>, grid, block, 0, st, a);
    else if (c <= kRegC)
        hipLaunchKernelGGL(seg_predict_kernel<kRegC>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(seg_predict_kernel<0>, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    if (!counts) return CAE_OK;
    return launch_seg_record(a.partial, n, a.bx, c, (long long)hw, reinterpret_cast<long long *>(counts), st);
}
