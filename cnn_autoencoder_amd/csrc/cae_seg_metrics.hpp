// The steps that the slide metrics share (cae_seg_predict.hip, cae_seg_hist.hip, cae_seg_objects.hip, cae_tiles.hip,
// cae_mask.hip): one text each for the per-pixel decisions, the block tally, the histogram add, the counted extent, the
// grid policy, the shape and bits checks, and the launchers of the two merge kernels (cae_seg_merge.hip).  The span a
// block of a plane histogram takes: cae_seg_span.hpp.  The key and bin of a logit: cae_seg_roc_key.hpp; the bin of a
// score: cae_seg_score_bin.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "cae_launch.hpp"
#include "cae_seg_span.hpp"

namespace cae {

// ---- shapes, grids, arguments (host) -----------------------------------------------------------------------------
constexpr int kMinBits = 8, kMaxBits = 14;  // 2^bits bins per class of a ROC histogram
constexpr int kBlocksTarget = 4096;         // blocks of a grid-stride launch at which more would only add partials
constexpr int kPartial = 4;                 // tallies per (image, block): one class tp tn fp fn; several tp tp_top sum -

inline bool bits_ok(int bits) { return bits >= kMinBits && bits <= kMaxBits; }
inline int refuse_bits(const char *who, int bits) {
    return fail(CAE_ERR_ARG, "%s: %d bits outside %d..%d", who, bits, kMinBits, kMaxBits);
}

// a pixel's cover is held in 16 bits (3 min(h, w) bounds it) and a label in 32
inline bool plane_fits(int h, int w) { return 3 * (long long)std::min(h, w) <= 65535 && (long long)h * w <= INT_MAX; }
inline bool plane_ok(int n, int h, int w) { return n >= 1 && h >= 1 && w >= 1 && plane_fits(h, w); }

inline bool misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// blocks per image: one per `per_block` items, fewer once the launch of n images has `cap` blocks, at least one
inline int blocks_for(int n, size_t items, size_t per_block, int cap) {
    const size_t most = std::max<size_t>(1, (size_t)cap / (size_t)std::max(n, 1));
    return (int)std::min((items + per_block - 1) / per_block, most);
}

// the cap of a histogram launch: a partial is 2^(bits+3) bytes or more, written and read again, and above 12 bits one
// block per CU of the 256 is all that runs at a time
inline int hist_blocks_target(int bits) { return bits > 12 ? 256 : 1024; }

// counts[n] = the record tp tn fp fn p tp_top of the bx partials [n][bx][kPartial]; several classes (c > 1) count
// `total` pixels, or with total < 0 what their tally 2 holds
int launch_seg_record(const unsigned long long *partial, int n, int bx, int c, long long total, long long *counts,
                      hipStream_t st);
// hist[m][2][2^bits] = the sum of the partials [n][bx][2][2^bits] per image (m = n) or over all of them (m = 1);
// W: uint32_t (16-byte aligned partials) or unsigned long long
template <typename W>
int launch_seg_histsum(const W *partial, int n, int bx, int per_image, int bits, long long *hist, hipStream_t st);

// the labelling of cae_seg_components (cae_seg_objects.hip) for any connectivity (4 or 8) and reading of the plane:
// foreground is any non-zero value (kAny), neighbours join only with equal values (kByValue), or foreground is where
// the plane is 0 (kZero).  The caller has checked shapes and pointers; workspace: components_workspace bytes, 8-byte
// aligned; n_objects may be NULL.  Labels: 0, or 1 + the smallest row-major index of the object
enum { kAny = 0, kByValue = 1, kZero = 2 };
size_t components_workspace(int n, int h, int w);
int launch_components(const uint8_t *target, const int32_t *extent, int n, int h, int w, int mode, int connectivity,
                      int32_t *labels, long long *n_objects, void *workspace, hipStream_t st);

// ---- device steps ------------------------------------------------------------------------------------------------
// the counted part of image n: (rows, cols), clamped to the plane
__device__ __forceinline__ void extent_of(const int32_t *extent, int n, int h, int w, int &rows, int &cols) {
    rows = h, cols = w;
    if (extent) {
        const auto clamped = [&](int i, int most) { return std::min(std::max(extent[2 * n + i], 0), most); };
        rows = clamped(0, h), cols = clamped(1, w);
    }
}

// floats in front of the first 16-byte aligned address at or behind p (p 4-byte aligned)
__device__ __forceinline__ size_t aligned_head(const float *p) { return span_head<4>(span_offset<4>(p)); }

// `EACH` counts from every lane that is `on` into a block's LDS histogram, `word` the lane's counter.  LEADS times over,
// the lanes of a wave that hold the word of the first waiting lane add once, by their number, before the rest add on
// their own: a slide's background puts most of a wave on one or two words, and 64 adds to one LDS word take 64 turns
template <uint32_t EACH, int LEADS>
__device__ __forceinline__ void hist_add(uint32_t *hist, bool on, uint32_t word) {
#pragma unroll
    for (int r = 0; r < LEADS; ++r) {
        if (on) {
            const uint32_t lead = __builtin_amdgcn_readfirstlane(word);
            const unsigned long long same = __ballot(word == lead);  // the lanes of this branch only; the first is among them
            if (word == lead) {
                if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1)
                    atomicAdd(&hist[lead], EACH * (uint32_t)__popcll(same));
                on = false;
            }
        }
    }
    if (on) atomicAdd(&hist[word], EACH);
}

// a lane's tallies.  W = unsigned where every pixel adds 1 (a lane sees hw / (256 bx) + 7 pixels and hw floats fit the
// device's memory), unsigned long long where it adds its cover: no count of pixels times 65535 leaves 64 bits
template <typename W>
struct Tally {
    W v[kPartial];
};

// tally `threadIdx.x` of the block in the lanes threadIdx.x < kPartial: over the wave by shuffles, over the block through
// LDS, in wave order
template <int THREADS, typename W>
__device__ __forceinline__ unsigned long long block_tally_sum(const Tally<W> &ty) {
    __shared__ unsigned long long wave_sum[THREADS / 64][kPartial];
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kPartial; ++j) {
        unsigned long long s = ty.v[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
        if ((tid & 63) == 0) wave_sum[tid >> 6][j] = s;
    }
    __syncthreads();
    unsigned long long s = 0;
    if (tid < kPartial) {
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) s += wave_sum[w][tid];
    }
    return s;
}

// every (image, block) writes its partial, work or not
template <int THREADS, typename W>
__device__ __forceinline__ void block_tally_store(const Tally<W> &ty, unsigned long long *partial) {
    const unsigned long long s = block_tally_sum<THREADS>(ty);
    if (threadIdx.x < kPartial) partial[(size_t)blockIdx.x * kPartial + threadIdx.x] = s;
}

// The decision contract, once.  One class: on above the threshold.  Several: the class is the first of the largest
// logits, and the target's rank counts the logits that come before its own in that order.  NaN is never above anything.
__device__ __forceinline__ bool above(float x, float t) { return x > t; }
__device__ __forceinline__ bool before(float v, int c, float lt, int tgt) { return v > lt || (c < tgt && v == lt); }

// one pixel of one class; `add`: 1 or its cover.  x becomes its score if `want`
template <typename W>
__device__ __forceinline__ uint8_t decide_binary(float &x, float t, int tgt, bool want, W add, Tally<W> &ty) {
    const bool on = above(x, t);
    if (tgt >= 0) {
        const bool pos = tgt > 0;
        ty.v[0] += on && pos ? add : 0;
        ty.v[1] += !on && !pos ? add : 0;
        ty.v[2] += on && !pos ? add : 0;
        ty.v[3] += !on && pos ? add : 0;
    }
    if (want) {
        // e in (0, 1]: no overflow, and the rounding of the argument costs |x| e^-|x| 2^-24 absolute at most
        const float e = __expf(-fabsf(x));
        const float r = 1.0f / (1.0f + e);
        x = x >= 0.f ? r : e * r;
    }
    return on;
}

// one pixel of C classes, its planes streamed; with SCORES its scores to sc (no exponential otherwise) -> class index
template <bool SCORES, typename W>
__device__ __forceinline__ uint8_t decide_stream(const float *lg, float *sc, size_t hw, size_t p, int C, int tgt, int k,
                                                 W add, Tally<W> &ty) {
    float best = lg[p];
    int idx = 0;
    for (int c = 1; c < C; ++c) {
        const float v = lg[(size_t)c * hw + p];
        if (above(v, best)) {  // strict: idx stays in 0..C-1
            best = v;
            idx = c;
        }
    }
    if (tgt < 0 && !SCORES) return (uint8_t)idx;
    const bool ranked = tgt >= 0 && tgt < C;  // the only use of the target as an index, behind its bound
    const float lt = ranked ? lg[(size_t)tgt * hw + p] : 0.f;
    float s = 0.f;
    int rank = 0;
    for (int c = 0; c < C; ++c) {
        const float v = lg[(size_t)c * hw + p];
        if constexpr (SCORES) s += __expf(v - best);
        rank += before(v, c, lt, tgt);
    }
    if (tgt >= 0) {
        ty.v[0] += idx == tgt ? add : 0;
        ty.v[1] += ranked && rank < k ? add : 0;
    }
    if constexpr (SCORES) {
        const float r = 1.0f / s;
        for (int c = 0; c < C; ++c) sc[(size_t)c * hw + p] = __expf(lg[(size_t)c * hw + p] - best) * r;
    }
    return (uint8_t)idx;
}

}  // namespace cae
