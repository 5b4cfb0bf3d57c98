// The border weight map of a label plane (include/cae_hip.h, "Weight map of a label plane"): squared Euclidean distances
// to the nearest and to the second-nearest object, and the U-Net weight made of them, with their launchers.
//
// cae_seg_object_distances: two passes over records (squared row distance, label), a label of 0 standing for "none"
// with the distance kNone, above every real sum, so that an empty record loses every comparison without a branch.
// (1) column pass, one lane per column: a downward scan keeps the latest label and the latest different label with
// their rows and stores them per pixel; the upward scan keeps the same two below, merges the up to four candidates
// into the pixel's two nearest distinct labels of its column and stores that record in place of the first.  (2) row
// pass, one lane per pixel: the records of the pixel's row pass through LDS in chunks of kChunk columns, every lane
// reading the same record in a turn (a broadcast), and each adds its squared column distance and keeps the smallest
// sum, its label and the smallest sum of another label.  Both results are minima over fixed sets of integers: they do
// not depend on the order in which the candidates come.  No atomics; no block waits for another.
//
// cae_seg_weight_map: one lane per pixel, fp32 arithmetic on the correctly rounded double roots of the two distances.
#include "cae_seg_metrics.hpp"

#include <cmath>

namespace cae {
namespace {

constexpr int kThreads = 256;
constexpr int kColThreads = 64;        // the column pass has n w lanes in all: small blocks spread them over the CUs
constexpr int kRows = 16;              // rows a column scan loads at a time
constexpr int kChunk = 256;           // columns of a row whose records stand in LDS at a time
constexpr int kMaxEdge = 32768;        // 2 (kMaxEdge - 1)^2 < kNone: every real sum stays below "none"
constexpr uint32_t kNone = 0x7FFFFFFFu;  // the distance of an empty record; kNone + (kMaxEdge - 1)^2 < 2^32

// the two nearest candidates of distinct labels: d0 <= d1 always, l1 != l0 or empty
struct Two {
    uint32_t d0, d1;
    int l0, l1;
};

__device__ __forceinline__ Two two_none() { return {kNone, kNone, 0, 0}; }

// the two-slot rule: a nearer candidate of the first label only moves the first; one of another label takes the
// second place, or the first and pushes the first down
__device__ __forceinline__ void push(Two &t, uint32_t d, int l) {
    const bool nearer = d < t.d0, other = l != t.l0;
    const uint32_t second = nearer ? t.d0 : d;  // what the second place would hold: the farther of the two
    if (other && second < t.d1) {
        t.d1 = second;
        t.l1 = nearer ? t.l0 : l;
    }
    if (nearer) t.d0 = d, t.l0 = l;
}

// the scan's state: rows of the latest label and of the latest different label (valid where the label is not 0)
struct Latest {
    int l0, l1, y0, y1;
};

__device__ __forceinline__ void see(Latest &s, int l, int y) {
    if (l == 0) return;
    if (l != s.l0) s.l1 = s.l0, s.y1 = s.y0, s.l0 = l;
    s.y0 = y;
}

__device__ __forceinline__ uint32_t sq(int d) { return (uint32_t)(d * d); }  // |d| < kMaxEdge

// records[n][h][w] = (d0, l0, d1, l1): squared row distances and labels of the two nearest distinct labels of the column
// The scans step through kRows rows at a time, their loads issued together: the state is the only chain between rows.
__global__ __launch_bounds__(kColThreads) void wd_column_kernel(const int *__restrict__ labels, int4 *records, int h, int w,
                                                                size_t total_cols) {
    const size_t col = (size_t)blockIdx.x * kColThreads + threadIdx.x;
    if (col >= total_cols) return;
    const size_t off = (col / w) * ((size_t)h * w) + col % w;
    const int *lab = labels + off;
    int4 *rec = records + off;
    Latest s = {0, 0, 0, 0};
    for (int yb = 0; yb < h; yb += kRows) {
        int l[kRows];
#pragma unroll
        for (int j = 0; j < kRows; ++j) l[j] = yb + j < h ? lab[(size_t)(yb + j) * w] : 0;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int y = yb + j;
            if (y >= h) break;
            see(s, l[j], y);
            rec[(size_t)y * w] =
                make_int4(s.l0 ? (int)sq(y - s.y0) : (int)kNone, s.l0, s.l1 ? (int)sq(y - s.y1) : (int)kNone, s.l1);
        }
    }
    s = {0, 0, 0, 0};
    for (int yb = (h - 1) / kRows * kRows; yb >= 0; yb -= kRows) {
        int l[kRows];
        int4 up[kRows];  // this lane's own stores of the first scan
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const bool in = yb + j < h;
            l[j] = in ? lab[(size_t)(yb + j) * w] : 0;
            up[j] = in ? rec[(size_t)(yb + j) * w] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = kRows - 1; j >= 0; --j) {
            const int y = yb + j;
            if (y >= h) continue;
            see(s, l[j], y);
            Two t = two_none();
            push(t, (uint32_t)up[j].x, up[j].y);
            push(t, (uint32_t)up[j].z, up[j].w);
            push(t, s.l0 ? sq(s.y0 - y) : kNone, s.l0);
            push(t, s.l1 ? sq(s.y1 - y) : kNone, s.l1);
            rec[(size_t)y * w] = make_int4((int)t.d0, t.l0, (int)t.d1, t.l1);
        }
    }
}

// d2[n][2][h][w] from the records of the pixel's row; a block holds THREADS consecutive columns of one row
template <int THREADS>
__global__ __launch_bounds__(THREADS) void wd_row_kernel(const int4 *records, int *d2, int h, int w, int segs) {
    __shared__ int4 rec[kChunk];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x / segs;  // n h rows in all
    const int x = (int)(blockIdx.x % segs) * THREADS + tid;
    const int4 *src = records + row * w;
    uint32_t b0 = ~0u, b1 = ~0u;  // b0 <= b1 throughout
    int l0 = 0;
    for (int c0 = 0; c0 < w; c0 += kChunk) {
        const int cnt = std::min(kChunk, w - c0);
        __syncthreads();  // the last chunk has been read by every lane
        for (int j = tid; j < cnt; j += THREADS) rec[j] = src[c0 + j];
        __syncthreads();
        const int dx0 = x - c0;
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const int4 r = rec[j];
            const int dx = dx0 - j;  // |dx| < 2^24 also in the lanes beyond the row
            const uint32_t e = (uint32_t)__mul24(dx, dx);
            const uint32_t c[2] = {e + (uint32_t)r.x, e + (uint32_t)r.z};
            const int l[2] = {r.y, r.w};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                // the two-slot rule without the second label: b1 = min(b1, the farther of b0 and c) for another label
                const bool nearer = c[k] < b0;
                const uint32_t second = std::min(b1, std::max(b0, c[k]));
                b1 = l[k] != l0 ? second : b1;
                l0 = nearer ? l[k] : l0;
                b0 = std::min(b0, c[k]);
            }
        }
    }
    if (x >= w) return;
    const size_t hw = (size_t)h * w;
    int *out = d2 + (row / h) * 2 * hw + (row % h) * w + x;
    out[0] = b0 < kNone ? (int)b0 : -1;
    out[hw] = b1 < kNone ? (int)b1 : -1;
}

struct MapArgs {
    const float *target;
    const int *d2;
    const long long *n_objects;
    const float *class_weights;
    float *out;
    int *flag;
    size_t hw;
    int n_class_weights, bx;
    float sigma_2, w_0;
};

// scipy's float64 distance cast to float32
__device__ __forceinline__ float root(int d2) { return (float)sqrt((double)d2); }

__global__ __launch_bounds__(kThreads) void wd_map_kernel(MapArgs a) {
#pragma clang fp contract(off)  // every product and sum rounds to fp32 on its own, as the host's float32 arrays do
    const int n = blockIdx.x / a.bx;
    const size_t hw = a.hw, stride = (size_t)a.bx * kThreads;
    const float *tg = a.target + (size_t)n * hw;
    const int *d2 = a.d2 + (size_t)n * 2 * hw;
    float *out = a.out + (size_t)n * 2 * hw;
    const long long objects = a.n_objects[n];
    bool bad = false;
    for (size_t p = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; p < hw; p += stride) {
        const float t = tg[p];
        float wgt = NAN;
        if (t >= 0.f && t < (float)a.n_class_weights) {  // false for NaN; the only use of the target as an index
            wgt = a.class_weights[(int)t];
            if (objects > 0) {
                float d = root(d2[p]);
                if (objects > 1) d = d + root(d2[hw + p]);
                const float e = expf(-((d * d) / a.sigma_2));
                wgt = wgt + a.w_0 * e;
            }
        } else {
            bad = true;
        }
        out[p] = wgt;
        out[hw + p] = t;
    }
    if (bad) *a.flag = 1;
}

bool edges_ok(int h, int w) {
    return h >= 1 && w >= 1 && h <= kMaxEdge && w <= kMaxEdge && (long long)h * w <= INT_MAX;
}

// blocks of the row pass: rows x segments of `threads` columns
size_t row_blocks(int n, int h, int w, int threads) { return (size_t)n * h * ((w + threads - 1) / threads); }

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" size_t cae_seg_object_distances_workspace(int n, int h, int w) {
    if (n < 1 || !edges_ok(h, w)) return 0;
    return (size_t)n * (size_t)h * (size_t)w * sizeof(int4);
}

extern "C" int cae_seg_object_distances(const int32_t *labels, int n, int h, int w, int32_t *d2, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_seg_object_distances: bad shape n=%d h=%d w=%d", n, h, w);
    if (!edges_ok(h, w))
        return fail(CAE_ERR_ARG, "cae_seg_object_distances: planes of %d x %d pixels are too large", h, w);
    if (n == 0) return CAE_OK;
    if (!labels || !d2) return fail(CAE_ERR_ARG, "cae_seg_object_distances: NULL labels or distances");
    if (misaligned(labels, 3) || misaligned(d2, 3))
        return fail(CAE_ERR_ARG, "cae_seg_object_distances: labels or distances not 4-byte aligned");
    const size_t need = cae_seg_object_distances_workspace(n, h, w);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 15))
        return fail(CAE_ERR_ARG, "cae_seg_object_distances: workspace NULL, not 16-byte aligned or too small: %zu bytes needed", need);
    const int threads = w <= 64 ? 64 : kThreads;
    const size_t cols = (size_t)n * w, blocks = row_blocks(n, h, w, threads);
    if (blocks > (size_t)INT_MAX)
        return fail(CAE_ERR_ARG, "cae_seg_object_distances: %d planes of %d x %d are too many for one call", n, h, w);
    int4 *records = static_cast<int4 *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wd_column_kernel, dim3((unsigned)((cols + kColThreads - 1) / kColThreads)), dim3(kColThreads), 0, st,
                       labels, records, h, w, cols);
    HIP_TRY(hipGetLastError());
    const int segs = (w + threads - 1) / threads;
    if (threads == 64)
        hipLaunchKernelGGL(wd_row_kernel<64>, dim3((unsigned)blocks), dim3(64), 0, st, records, d2, h, w, segs);
    else
        hipLaunchKernelGGL(wd_row_kernel<kThreads>, dim3((unsigned)blocks), dim3(kThreads), 0, st, records, d2, h, w, segs);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" int cae_seg_weight_map(const float *target, const int32_t *d2, const int64_t *n_objects,
                                  const float *class_weights, int n_class_weights, float sigma_2, float w_0, int n,
                                  size_t hw, float *out, int *flag, void *stream) {
    if (n < 0 || hw < 1) return fail(CAE_ERR_ARG, "cae_seg_weight_map: bad shape n=%d hw=%zu", n, hw);
    if (n_class_weights < 1) return fail(CAE_ERR_ARG, "cae_seg_weight_map: %d class weights", n_class_weights);
    if (!(std::isfinite(sigma_2) && sigma_2 > 0.f))
        return fail(CAE_ERR_ARG, "cae_seg_weight_map: sigma_2 %g is not finite and positive", (double)sigma_2);
    if (n == 0) return CAE_OK;
    if (!target || !d2 || !n_objects || !class_weights || !out || !flag)
        return fail(CAE_ERR_ARG, "cae_seg_weight_map: NULL target, distances, n_objects, class_weights, out or flag");
    MapArgs a;
    a.target = target, a.d2 = d2, a.n_objects = reinterpret_cast<const long long *>(n_objects);
    a.class_weights = class_weights, a.out = out, a.flag = flag, a.hw = hw, a.n_class_weights = n_class_weights;
    a.bx = blocks_for(n, hw, kThreads, kBlocksTarget), a.sigma_2 = sigma_2, a.w_0 = w_0;
    hipLaunchKernelGGL(wd_map_kernel, dim3((unsigned)((size_t)n * a.bx)), dim3(kThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
