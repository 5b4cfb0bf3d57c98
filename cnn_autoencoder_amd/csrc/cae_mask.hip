// The tissue mask of a slide (include/cae_hip.h, "Tissue mask of a slide"): gray and its range, the 256-bin histogram
// behind the Otsu threshold, the threshold, 4- or 8-connected labels, the area filter, the disk test on squared
// distances and the box downscale, with their launchers.  The labelling is that of cae_seg_objects.hip
// (launch_components) and the distances are cae_seg_object_distances; what is here is what lies between them.
//
// Everything but the gray value is integer arithmetic, and the gray value is three float64 divisions, three products
// and two sums, each rounded on its own (no contraction): every result is a function of the input alone, whatever the
// launch shape or the order of execution.  Global and LDS atomics are integer min / max / add only.
//
// The elementwise kernels walk one plane per block row.  A lane takes 16 bytes of the narrower side at a time (4 pixels
// of gray, 16 of a uint8 plane) with 16-byte loads and stores where the plane's own addresses are 16-byte aligned (4-byte
// for the three-byte pixels of the image), and single elements otherwise and behind the last whole group.
#include "cae_seg_metrics.hpp"

namespace cae {
namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;                // bins of the histogram; one lane of a block owns one bin
constexpr uint32_t kFold = 16384;         // pixels a block adds into its 32-bit LDS bins before it folds them away
constexpr size_t kHistPerBlock = 65536;   // pixels per block of the histogram below the cap: four folds
constexpr int kHistBlocksTarget = 1024;
constexpr int kSumBits = 7;               // launch_seg_histsum sums tables of 2 << bits words
constexpr int kMaxFactor = 64;            // 64 x 64 x 255 stays far below 2^32

__device__ __forceinline__ bool aligned_to(const void *p, unsigned mask) {
    return (reinterpret_cast<uintptr_t>(p) & mask) == 0;
}

// ---- gray, min and max ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double gray_of(unsigned R, unsigned G, unsigned B) {
#pragma clang fp contract(off)
    const double r = (double)R / 255.0, g = (double)G / 255.0, b = (double)B / 255.0;
    return (0.2125 * r + 0.7154 * g) + 0.0721 * b;
}

__global__ __launch_bounds__(64) void mask_range_init_kernel(unsigned long long *minmax, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) minmax[2 * i] = ~0ull, minmax[2 * i + 1] = 0ull;
}

// gray is never negative, so its bit pattern orders as an unsigned integer: the range is an integer min / max
__global__ __launch_bounds__(kThreads) void mask_gray_kernel(const uint8_t *img, double *gray, unsigned long long *minmax,
                                                             size_t hw, int bx) {
    const int n = blockIdx.x / bx, tid = threadIdx.x;
    const uint8_t *src = img + (size_t)n * hw * 3;
    double *dst = gray + (size_t)n * hw;
    const size_t first = (size_t)(blockIdx.x % bx) * kThreads + tid, stride = (size_t)bx * kThreads;
    unsigned long long lo = ~0ull, hi = 0ull;
    const auto put = [&](size_t p, double v) {
        dst[p] = v;
        const unsigned long long k = (unsigned long long)__double_as_longlong(v);
        lo = std::min(lo, k), hi = std::max(hi, k);
    };
    size_t done = 0;
    if (aligned_to(src, 3) && aligned_to(dst, 15)) {
        const size_t groups = hw / 4;
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
        for (size_t g = first; g < groups; g += stride) {
            const uint32_t a = s32[3 * g], b = s32[3 * g + 1], c = s32[3 * g + 2];  // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            double v[4];
            v[0] = gray_of(a & 255, (a >> 8) & 255, (a >> 16) & 255);
            v[1] = gray_of(a >> 24, b & 255, (b >> 8) & 255);
            v[2] = gray_of((b >> 16) & 255, b >> 24, c & 255);
            v[3] = gray_of((c >> 8) & 255, (c >> 16) & 255, c >> 24);
            double2 *d = reinterpret_cast<double2 *>(dst + 4 * g);
            d[0] = make_double2(v[0], v[1]);
            d[1] = make_double2(v[2], v[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long k = (unsigned long long)__double_as_longlong(v[j]);
                lo = std::min(lo, k), hi = std::max(hi, k);
            }
        }
        done = groups * 4;
    }
    for (size_t p = done + first; p < hw; p += stride) put(p, gray_of(src[3 * p], src[3 * p + 1], src[3 * p + 2]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = std::min(lo, (unsigned long long)__shfl_down(lo, d, 64));
        hi = std::max(hi, (unsigned long long)__shfl_down(hi, d, 64));
    }
    __shared__ unsigned long long wave_lo[kThreads / 64], wave_hi[kThreads / 64];
    if ((tid & 63) == 0) wave_lo[tid >> 6] = lo, wave_hi[tid >> 6] = hi;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kThreads / 64; ++k) lo = std::min(lo, wave_lo[k]), hi = std::max(hi, wave_hi[k]);
        if (lo <= hi) {  // the block saw a pixel
            atomicMin(minmax + 2 * n, lo);
            atomicMax(minmax + 2 * n + 1, hi);
        }
    }
}

// ---- histogram -----------------------------------------------------------------------------------------------------
// numpy.histogram's bin of x for 256 equal bins over [e[0], e[256]]: the scaled estimate, then numpy's two corrections
// against the edges themselves
__device__ __forceinline__ int bin_of(double x, double lo, double scale, const double *e) {
#pragma clang fp contract(off)
    int idx = (int)((x - lo) * scale);
    idx = std::min(std::max(idx, 0), kBins - 1);  // 256 (x == hi) becomes 255; nothing else leaves the range
    if (x < e[idx] && idx > 0) idx -= 1;
    if (x >= e[idx + 1] && idx != kBins - 1) idx += 1;
    return idx;
}

// partial[n][bx][256]: the counts of the block's share of plane n; lane t of the block owns bin t
__global__ __launch_bounds__(kThreads) void mask_hist_kernel(const double *gray, const double *edges,
                                                             unsigned long long *partial, size_t hw, int bx) {
    static_assert(kThreads == kBins, "one lane per bin");
    __shared__ double e[kBins + 1];
    __shared__ uint32_t hist[kBins];
    const int n = blockIdx.x / bx, tid = threadIdx.x;
    const double *g = gray + (size_t)n * hw;
    for (int i = tid; i <= kBins; i += kThreads) e[i] = edges[(size_t)n * (kBins + 1) + i];
    hist[tid] = 0;
    __syncthreads();
    const double lo = e[0];
    double scale;
    {
#pragma clang fp contract(off)
        scale = 256.0 / (e[kBins] - lo);
    }
    size_t per_block = (hw + bx - 1) / bx;
    per_block += per_block & 1;  // even: a block starts on a pair of the plane
    const size_t p0 = std::min(hw, (size_t)(blockIdx.x % bx) * per_block), p1 = std::min(hw, p0 + per_block);
    const bool wide = aligned_to(g, 15);
    unsigned long long mine = 0;
    for (size_t c0 = p0; c0 < p1; c0 += kFold) {
        const size_t c1 = std::min(p1, c0 + kFold);  // at most kFold pixels: far below 2^32 a bin
        if (wide) {
            const size_t pairs = (c1 - c0) / 2;  // c0 is even
            const double2 *g2 = reinterpret_cast<const double2 *>(g + c0);
            for (size_t i = tid; i < pairs; i += kThreads) {
                const double2 v = g2[i];
                atomicAdd(&hist[bin_of(v.x, lo, scale, e)], 1u);
                atomicAdd(&hist[bin_of(v.y, lo, scale, e)], 1u);
            }
            if (tid == 0 && ((c1 - c0) & 1)) atomicAdd(&hist[bin_of(g[c1 - 1], lo, scale, e)], 1u);
        } else {
            for (size_t p = c0 + tid; p < c1; p += kThreads) atomicAdd(&hist[bin_of(g[p], lo, scale, e)], 1u);
        }
        __syncthreads();
        mine += hist[tid];  // the fold: 32-bit bin into the lane's 64-bit sum
        hist[tid] = 0;
        __syncthreads();
    }
    partial[(size_t)blockIdx.x * kBins + tid] = mine;  // every (plane, block) writes its partial, work or not
}

// ---- 16 pixels of a uint8 plane from 16 elements of T ---------------------------------------------------------------
// out[n][p] = f(n, src_n[p]) over hw pixels of each plane, src_n = src + n * src_pitch
template <typename T, typename F>
__device__ __forceinline__ void map_plane(const T *src, size_t src_pitch, uint8_t *out, size_t hw, int bx, F f) {
    const int n = blockIdx.x / bx;
    const T *s = src + (size_t)n * src_pitch;
    uint8_t *dst = out + (size_t)n * hw;
    const size_t first = (size_t)(blockIdx.x % bx) * kThreads + threadIdx.x, stride = (size_t)bx * kThreads;
    size_t done = 0;
    if (aligned_to(s, 15) && aligned_to(dst, 15)) {
        const size_t groups = hw / 16;
        for (size_t g = first; g < groups; g += stride) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(s + 16 * g);
            uint4 v[sizeof(T)];
#pragma unroll
            for (int k = 0; k < (int)sizeof(T); ++k) v[k] = s4[k];
            const T *t = reinterpret_cast<const T *>(v);
            uint32_t word[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) word[j / 4] |= (uint32_t)(f(n, t[j]) ? 1u : 0u) << (8 * (j % 4));
            *reinterpret_cast<uint4 *>(dst + 16 * g) = make_uint4(word[0], word[1], word[2], word[3]);
        }
        done = groups * 16;
    }
    for (size_t p = done + first; p < hw; p += stride) dst[p] = f(n, s[p]) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void mask_threshold_kernel(const double *gray, const double *thr, uint8_t *out,
                                                                  size_t hw, int bx) {
    map_plane(gray, hw, out, hw, bx, [thr](int n, double x) { return x <= thr[n]; });
}

// d2: (n, 2, hw), plane 0 read
__global__ __launch_bounds__(kThreads) void mask_within_kernel(const int *d2, int r2, uint8_t *out, size_t hw, int bx) {
    map_plane(d2, 2 * hw, out, hw, bx, [r2](int, int d) { return d >= 0 && d <= r2; });
}

// ---- area filter ---------------------------------------------------------------------------------------------------
struct AreaArgs {
    const int *labels;
    int *area;  // [n][hw], used at root pixels only
    uint8_t *plane;
    int *wide;  // [n][hw] or NULL: the plane as int32
    size_t hw;
    int bx, min_area, set_value;
};

// a label that names a root pixel of its plane -> that pixel's index, else -1: no label is an index before this
__device__ __forceinline__ long long root_of(const int *lab, size_t hw, int l) {
    return (l >= 1 && (size_t)l <= hw && lab[l - 1] == l) ? (long long)l - 1 : -1;
}

__global__ __launch_bounds__(kThreads) void mask_area_init_kernel(AreaArgs a) {
    const int n = blockIdx.x / a.bx;
    const size_t off = (size_t)n * a.hw, stride = (size_t)a.bx * kThreads;
    for (size_t i = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; i < a.hw; i += stride)
        if (a.labels[off + i] == (int)i + 1) a.area[off + i] = 0;
}

// A wave walks kSegments consecutive segments of 64 pixels of the plane.  Inside a segment the first lane of every run
// of one label adds the run's length; the run that reaches the segment's end is carried (label and length, the same in
// every lane) and grows while the next segments begin with its label, so a component of millions of pixels gets one
// add per 64 kSegments of them and not one per wave instruction.  All adds are integer: exact in any order.
constexpr int kSegments = 16;

__global__ __launch_bounds__(kThreads) void mask_area_count_kernel(AreaArgs a) {
    const int n = blockIdx.x / a.bx, lane = threadIdx.x & 63;
    const size_t off = (size_t)n * a.hw, hw = a.hw;
    const int *lab = a.labels + off;
    int *area = a.area + off;
    const auto add = [&](int l, int len) {  // (called by one lane)
        const long long r = root_of(lab, hw, l);
        if (r >= 0) atomicAdd(area + r, len);
    };
    const size_t chunk_px = (size_t)64 * kSegments, chunks = (hw + chunk_px - 1) / chunk_px;
    const size_t waves = (size_t)a.bx * (kThreads / 64);
    for (size_t c = (size_t)(blockIdx.x % a.bx) * (kThreads / 64) + (threadIdx.x >> 6); c < chunks; c += waves) {  // whole waves
        int held = 0, held_len = 0;  // the carried run; label 0 carries nothing
        for (int s = 0; s < kSegments; ++s) {
            const size_t i = c * chunk_px + (size_t)s * 64 + lane;
            const int l = i < hw ? lab[i] : 0;
            const int left = __shfl_up(l, 1, 64);
            const bool start = lane == 0 || left != l;
            const unsigned long long starts = __ballot(start);  // bit 0 is always set
            const int first = __shfl(l, 0, 64), last = __shfl(l, 63, 64);
            const int last_start = 63 - __clzll((long long)starts);
            const int first_len = (starts >> 1) ? __ffsll((long long)(starts >> 1)) : 64;
            if (start && l != 0 && lane != 0 && lane != last_start) {  // a run strictly inside the segment
                const unsigned long long behind = starts >> (lane + 1);  // lane < last_start <= 63
                add(l, __ffsll((long long)behind));
            }
            if (first != held) {
                if (lane == 0 && held != 0) add(held, held_len);
                held = first, held_len = 0;
            }
            held_len += first_len;
            if (first_len < 64) {  // another run ends the segment (last_start >= first_len > 0): it is carried on
                if (lane == 0 && held != 0) add(held, held_len);
                held = last, held_len = 64 - last_start;
            }
        }
        if (lane == 0 && held != 0) add(held, held_len);
    }
}

__global__ __launch_bounds__(kThreads) void mask_area_write_kernel(AreaArgs a) {
    const int n = blockIdx.x / a.bx;
    const size_t off = (size_t)n * a.hw, stride = (size_t)a.bx * kThreads;
    const int *lab = a.labels + off;
    for (size_t i = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; i < a.hw; i += stride) {
        const int l = lab[i];
        int v = a.plane[off + i] != 0;
        if (l != 0) {
            const long long r = root_of(lab, a.hw, l);
            if (r >= 0 && a.area[off + r] < a.min_area) a.plane[off + i] = (uint8_t)(v = a.set_value);
        }
        if (a.wide) a.wide[off + i] = v;
    }
}

// ---- downscale -----------------------------------------------------------------------------------------------------
struct ScaleArgs {
    const uint8_t *img;
    uint8_t *out;
    size_t row_pitch, plane_pitch;  // bytes between rows / images of img
    int h, w, f, oh, ow, bx;
};

// one lane per output pixel: the rounded mean of the real pixels of its f x f block, per channel
template <int C>
__global__ __launch_bounds__(kThreads) void mask_downscale_kernel(ScaleArgs a) {
    const int n = blockIdx.x / a.bx;
    const size_t opix = (size_t)a.oh * a.ow, stride = (size_t)a.bx * kThreads;
    const uint8_t *src = a.img + (size_t)n * a.plane_pitch;
    uint8_t *dst = a.out + (size_t)n * opix * C;
    const int f = a.f;
    // 16-byte loads: whole blocks whose rows are runs of 16 C bytes that start on a 16-byte address
    constexpr int kUnit = C == 3 ? 48 : 16;
    const bool wide = (f * C) % kUnit == 0 && a.row_pitch % 16 == 0 && a.plane_pitch % 16 == 0 && aligned_to(a.img, 15);
    for (size_t o = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; o < opix; o += stride) {
        const int oy = (int)(o / a.ow), ox = (int)(o % a.ow);
        const int y0 = oy * f, x0 = ox * f;
        const int rows = std::min(f, a.h - y0), cols = std::min(f, a.w - x0);
        uint32_t sum[C];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = 0;
        const uint8_t *blk = src + (size_t)y0 * a.row_pitch + (size_t)x0 * C;
        if (wide && cols == f) {
            for (int y = 0; y < rows; ++y) {
                const uint4 *row = reinterpret_cast<const uint4 *>(blk + (size_t)y * a.row_pitch);
                for (int u = 0; u < f * C / kUnit; ++u) {
                    uint4 v[kUnit / 16];
#pragma unroll
                    for (int k = 0; k < kUnit / 16; ++k) v[k] = row[u * (kUnit / 16) + k];
                    const uint32_t *wd = reinterpret_cast<const uint32_t *>(v);
#pragma unroll
                    for (int j = 0; j < kUnit; ++j) sum[j % C] += (wd[j / 4] >> (8 * (j % 4))) & 255u;
                }
            }
        } else {
            for (int y = 0; y < rows; ++y) {
                const uint8_t *row = blk + (size_t)y * a.row_pitch;
                for (int x = 0; x < cols; ++x) {
#pragma unroll
                    for (int c = 0; c < C; ++c) sum[c] += row[x * C + c];
                }
            }
        }
        const uint32_t cnt = (uint32_t)(rows * cols);
#pragma unroll
        for (int c = 0; c < C; ++c) dst[o * C + c] = (uint8_t)((2 * sum[c] + cnt) / (2 * cnt));
    }
}

int plane_blocks(int n, size_t items, size_t per_lane) {
    return blocks_for(n, (items + per_lane - 1) / per_lane, kThreads, kBlocksTarget);
}

int hist_blocks(int n, size_t hw) { return blocks_for(n, hw, kHistPerBlock, kHistBlocksTarget); }

// the planes of the reused labelling and distance kernels
bool mask_plane_fits(int h, int w) { return plane_fits(h, w) && h <= 32768 && w <= 32768; }

}  // namespace
}  // namespace cae

using namespace cae;

extern "C" int cae_mask_gray(const uint8_t *img, int n, size_t hw, double *gray, double *minmax, void *stream) {
    if (n < 0 || hw < 1 || hw > (size_t)INT_MAX) return fail(CAE_ERR_ARG, "cae_mask_gray: bad shape n=%d hw=%zu", n, hw);
    if (n == 0) return CAE_OK;
    if (!img || !gray || !minmax) return fail(CAE_ERR_ARG, "cae_mask_gray: NULL image, gray or minmax");
    if (misaligned(gray, 7) || misaligned(minmax, 7)) return fail(CAE_ERR_ARG, "cae_mask_gray: gray or minmax not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *mm = reinterpret_cast<unsigned long long *>(minmax);
    hipLaunchKernelGGL(mask_range_init_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, mm, n);
    HIP_TRY(hipGetLastError());
    const int bx = plane_blocks(n, hw, 4);
    hipLaunchKernelGGL(mask_gray_kernel, dim3((unsigned)((size_t)n * bx)), dim3(kThreads), 0, st, img, gray, mm, hw, bx);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" size_t cae_mask_hist_workspace(int n, size_t hw) {
    if (n < 1 || hw < 1 || hw > (size_t)INT_MAX) return 0;
    return (size_t)n * hist_blocks(n, hw) * kBins * sizeof(unsigned long long);
}

extern "C" size_t cae_mask_hist_fold(void) { return kFold; }

extern "C" int cae_mask_hist(const double *gray, const double *edges, int n, size_t hw, int64_t *counts, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (n < 0 || hw < 1 || hw > (size_t)INT_MAX) return fail(CAE_ERR_ARG, "cae_mask_hist: bad shape n=%d hw=%zu", n, hw);
    if (n == 0) return CAE_OK;
    if (!gray || !edges || !counts) return fail(CAE_ERR_ARG, "cae_mask_hist: NULL gray, edges or counts");
    if (misaligned(gray, 7) || misaligned(edges, 7) || misaligned(counts, 7))
        return fail(CAE_ERR_ARG, "cae_mask_hist: gray, edges or counts not 8-byte aligned");
    const size_t need = cae_mask_hist_workspace(n, hw);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 7))
        return fail(CAE_ERR_ARG, "cae_mask_hist: workspace NULL, not 8-byte aligned or too small: %zu bytes needed", need);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *partial = static_cast<unsigned long long *>(workspace);
    const int bx = hist_blocks(n, hw);
    hipLaunchKernelGGL(mask_hist_kernel, dim3((unsigned)((size_t)n * bx)), dim3(kThreads), 0, st, gray, edges, partial, hw, bx);
    HIP_TRY(hipGetLastError());
    // the partials of a plane summed in a fixed order (seg_histsum_kernel, cae_seg_merge.hip: 256 words are the table of "7 bits")
    return launch_seg_histsum(partial, n, bx, 1, kSumBits, reinterpret_cast<long long *>(counts), st);
}

extern "C" int cae_mask_threshold(const double *gray, const double *thr, int n, size_t hw, uint8_t *out, void *stream) {
    if (n < 0 || hw < 1 || hw > (size_t)INT_MAX) return fail(CAE_ERR_ARG, "cae_mask_threshold: bad shape n=%d hw=%zu", n, hw);
    if (n == 0) return CAE_OK;
    if (!gray || !thr || !out) return fail(CAE_ERR_ARG, "cae_mask_threshold: NULL gray, thresholds or plane");
    if (misaligned(gray, 7) || misaligned(thr, 7)) return fail(CAE_ERR_ARG, "cae_mask_threshold: gray or thresholds not 8-byte aligned");
    const int bx = plane_blocks(n, hw, 16);
    hipLaunchKernelGGL(mask_threshold_kernel, dim3((unsigned)((size_t)n * bx)), dim3(kThreads), 0, (hipStream_t)stream, gray, thr,
                       out, hw, bx);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" size_t cae_mask_label_workspace(int n, int h, int w) {
    return mask_plane_fits(h, w) ? components_workspace(n, h, w) : 0;
}

extern "C" int cae_mask_label(const uint8_t *plane, int n, int h, int w, int connectivity, int of_zero, int32_t *labels,
                              void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_mask_label: bad shape n=%d h=%d w=%d", n, h, w);
    if (!mask_plane_fits(h, w)) return fail(CAE_ERR_ARG, "cae_mask_label: planes of %d x %d pixels are too large", h, w);
    if (connectivity != 4 && connectivity != 8) return fail(CAE_ERR_ARG, "cae_mask_label: connectivity %d is neither 4 nor 8", connectivity);
    if (n == 0) return CAE_OK;
    if (!plane || !labels) return fail(CAE_ERR_ARG, "cae_mask_label: NULL plane or labels");
    if (misaligned(labels, 3)) return fail(CAE_ERR_ARG, "cae_mask_label: labels not 4-byte aligned");
    const size_t need = cae_mask_label_workspace(n, h, w);
    if (need == 0) return fail(CAE_ERR_ARG, "cae_mask_label: %d planes of %d x %d are too many for one call", n, h, w);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 7))
        return fail(CAE_ERR_ARG, "cae_mask_label: workspace NULL, not 8-byte aligned or too small: %zu bytes needed", need);
    return launch_components(plane, nullptr, n, h, w, of_zero ? kZero : kAny, connectivity, labels, nullptr, workspace,
                             (hipStream_t)stream);
}

extern "C" size_t cae_mask_area_workspace(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1 || !mask_plane_fits(h, w)) return 0;
    return (size_t)n * (size_t)h * (size_t)w * sizeof(int32_t);
}

extern "C" int cae_mask_area_filter(const int32_t *labels, int n, int h, int w, int min_area, int set_value,
                                    uint8_t *plane_inout, int32_t *wide_out, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_mask_area_filter: bad shape n=%d h=%d w=%d", n, h, w);
    if (!mask_plane_fits(h, w)) return fail(CAE_ERR_ARG, "cae_mask_area_filter: planes of %d x %d pixels are too large", h, w);
    if (min_area < 0 || (set_value != 0 && set_value != 1))
        return fail(CAE_ERR_ARG, "cae_mask_area_filter: min_area %d below 0 or set_value %d not 0 or 1", min_area, set_value);
    if (n == 0) return CAE_OK;
    if (!labels || !plane_inout) return fail(CAE_ERR_ARG, "cae_mask_area_filter: NULL labels or plane");
    if (misaligned(labels, 3) || (wide_out && misaligned(wide_out, 3)))
        return fail(CAE_ERR_ARG, "cae_mask_area_filter: labels or the int32 plane not 4-byte aligned");
    const size_t need = cae_mask_area_workspace(n, h, w);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 3))
        return fail(CAE_ERR_ARG, "cae_mask_area_filter: workspace NULL, not 4-byte aligned or too small: %zu bytes needed", need);
    AreaArgs a;
    a.labels = labels, a.area = static_cast<int *>(workspace), a.plane = plane_inout, a.wide = wide_out;
    a.hw = (size_t)h * w, a.bx = plane_blocks(n, a.hw, 1), a.min_area = min_area, a.set_value = set_value;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((size_t)n * a.bx)), block(kThreads);
    hipLaunchKernelGGL(mask_area_init_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mask_area_count_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mask_area_write_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" int cae_mask_within(const int32_t *d2, int n, size_t hw, int r2, uint8_t *out, void *stream) {
    if (n < 0 || hw < 1 || hw > (size_t)INT_MAX) return fail(CAE_ERR_ARG, "cae_mask_within: bad shape n=%d hw=%zu", n, hw);
    if (r2 < 0) return fail(CAE_ERR_ARG, "cae_mask_within: squared radius %d below 0", r2);
    if (n == 0) return CAE_OK;
    if (!d2 || !out) return fail(CAE_ERR_ARG, "cae_mask_within: NULL distances or plane");
    if (misaligned(d2, 3)) return fail(CAE_ERR_ARG, "cae_mask_within: distances not 4-byte aligned");
    const int bx = plane_blocks(n, hw, 16);
    hipLaunchKernelGGL(mask_within_kernel, dim3((unsigned)((size_t)n * bx)), dim3(kThreads), 0, (hipStream_t)stream, d2, r2, out,
                       hw, bx);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" int cae_mask_downscale(const uint8_t *img, int n, int h, int w, int c, size_t row_pitch, size_t plane_pitch,
                                  int f, uint8_t *out, void *stream) {
    if (n < 0 || h < 1 || w < 1 || (long long)h * w > INT_MAX)
        return fail(CAE_ERR_ARG, "cae_mask_downscale: bad shape n=%d h=%d w=%d", n, h, w);
    if (c < 1 || c > 4) return fail(CAE_ERR_ARG, "cae_mask_downscale: %d channels outside 1..4", c);
    if (f < 1 || f > kMaxFactor) return fail(CAE_ERR_ARG, "cae_mask_downscale: factor %d outside 1..%d", f, kMaxFactor);
    if (row_pitch < (size_t)w * c || (n > 1 && plane_pitch < (size_t)(h - 1) * row_pitch + (size_t)w * c))
        return fail(CAE_ERR_ARG, "cae_mask_downscale: pitches %zu / %zu are shorter than a row / an image", row_pitch, plane_pitch);
    if (n == 0) return CAE_OK;
    if (!img || !out) return fail(CAE_ERR_ARG, "cae_mask_downscale: NULL image or output");
    ScaleArgs a;
    a.img = img, a.out = out, a.row_pitch = row_pitch, a.plane_pitch = plane_pitch;
    a.h = h, a.w = w, a.f = f, a.oh = (h + f - 1) / f, a.ow = (w + f - 1) / f;
    a.bx = plane_blocks(n, (size_t)a.oh * a.ow, 1);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((size_t)n * a.bx)), block(kThreads);
    switch (c) {
        case 1: hipLaunchKernelGGL(mask_downscale_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(mask_downscale_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(mask_downscale_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(mask_downscale_kernel<4>, grid, block, 0, st, a); break;
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
