// Object-level metrics of a segmented slide (include/cae_hip.h, "Objects of a label plane"): connected-component
// labels, the cover of the objects' boxes, and cover-weighted counts and ROC histograms, with their launchers.
//
// cae_seg_components: union-find on the label array itself.  An entry holds 1 + the parent's row-major index (0 on
// background), and parent <= own index at every moment: an entry only ever falls (integer atomicMin), so every walk
// towards a root strictly descends and ends after at most own-index steps, whatever other lanes do meanwhile.  Launches:
// (1) every pixel points at the start of its row run inside its wave's 64 columns (a ballot, no memory traffic);
// (2) unions along the wave seams and with the row above, only where a neighbour in the same run does not make the same
// union; (3) every pixel walks to its root, which is the smallest index of its component whatever the order of the
// unions, and writes 1 + root; roots are counted per block; (4) the block counts are summed.  No lane waits for another.
// The same launches label for the tissue mask (cae_mask.hip, through launch_components): step (2) is one body with the
// connectivity as a template parameter -- 8 here, 4 (no unions across corners) in mask_merge4_kernel -- and the plane
// can be read as "zero is foreground", which labels the complement.
//
// cae_seg_object_cover: box limits in integer min / max arrays addressed by the root pixel (the root's row is the top
// row), one +-1 per box corner into a difference plane, row and column prefix sums.  All sums are integer: exact in any
// order.
//
// cae_seg_object_counts / _roc_hist: the tallies of cae_seg_predict and the histogram of cae_seg_roc_hist with every
// pixel counted cover times.  Tallies and partials are 64 bits wide throughout; the one 32-bit accumulator, the LDS
// histogram, is added into the block's 64-bit partial and cleared every kChunk = 65536 pixels: 65536 * 65535 < 2^32.
// The decisions, the block tally, the counted extent, the shape checks and the grid policy are those of the image-level
// metrics (cae_seg_metrics.hpp), and so are the two merge kernels behind the partials (cae_seg_merge.hip).
#include "cae_seg_metrics.hpp"
#include "cae_seg_roc_key.hpp"

namespace cae {
namespace {

constexpr int kThreads = 256;
constexpr int kHistThreads = 1024;
constexpr uint32_t kChunk = 65536;   // pixels a block adds into its 32-bit LDS words before it flushes them

struct Plane {
    int h, w, wseg;  // wseg: 64-column segments of a row
    int bx;          // blocks per image
};

// block and lane -> image n, pixel (y, x); x may lie beyond the row (x >= w) and y beyond the plane: a wave holds 64
// consecutive columns of one row
__device__ __forceinline__ void place(const Plane &p, int &n, int &y, int &x) {
    n = blockIdx.x / p.bx;
    const size_t slot = (size_t)(blockIdx.x % p.bx) * kThreads + threadIdx.x;
    const size_t row = (size_t)p.wseg * 64;
    y = (int)std::min<size_t>(slot / row, (size_t)p.h);
    x = (int)(slot % row);
}

__device__ __forceinline__ int load_entry(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above pixel i.  L[j] - 1 <= j always, so i strictly falls until it stands on a root
__device__ __forceinline__ int find_root(const int *L, int i) {
    for (;;) {
        const int p = load_entry(L + i) - 1;
        if (p >= i || p < 0) return i;  // p == i: a root (the other two never happen; the walk falls regardless)
        i = p;
    }
}

// joins the trees of pixels a and b: the larger root is hung below the smaller one.  Every turn either ends or
// continues from a strictly smaller a, so it ends
__device__ __forceinline__ void unite(int *L, int a, int b) {
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b, b = s;
        }
        const int old = atomicMin(L + a, b + 1);  // b < a: the entry falls
        if (old == a + 1) return;                 // a was a root and now hangs below b
        a = old - 1;                              // a had a parent already: that tree joins b's
    }
}

struct CompArgs {
    const uint8_t *target;
    const int32_t *extent;
    int *labels;
    unsigned long long *partial;  // [n][bx] roots per block
    Plane p;
    int by_value;  // kAny, kByValue or kZero
};

// value of (y, x) of a plane as the labelling sees it: 0 outside plane or extent; else 1 for any foreground (kAny), the
// pixel's value (kByValue), or 1 where the plane is 0 (kZero: the objects of the complement)
__device__ __forceinline__ int seen(const uint8_t *tg, int w, int rows, int cols, int by_value, int y, int x) {
    if (y < 0 || x < 0 || y >= rows || x >= cols) return 0;
    const int t = tg[(size_t)y * w + x];
    return by_value == kByValue ? t : ((t != 0) != (by_value == kZero));
}

__global__ __launch_bounds__(kThreads) void obj_init_kernel(CompArgs a) {
    int n, y, x, rows, cols;
    place(a.p, n, y, x);
    const int h = a.p.h, w = a.p.w;
    extent_of(a.extent, n, h, w, rows, cols);
    const size_t hw = (size_t)h * w;
    const uint8_t *tg = a.target + (size_t)n * hw;
    const bool inside = y < h && x < w;
    const int v = inside ? seen(tg, w, rows, cols, a.by_value, y, x) : 0;
    const int lane = threadIdx.x & 63;
    const int left = __shfl_up(v, 1, 64);
    const bool start = v == 0 || lane == 0 || left != v;  // background lanes break runs
    const unsigned long long starts = __ballot(start);
    if (!inside) return;
    int entry = 0;
    if (v) {
        const unsigned long long upto = starts & (~0ull >> (63 - lane));  // bit `lane` is set among them or below
        const int first = 63 - __clzll((long long)upto);                 // this lane's run starts here (lane 0 at most)
        entry = (int)((size_t)y * w + x) - (lane - first) + 1;
    }
    a.labels[(size_t)n * hw + (size_t)y * w + x] = entry;
}

// CONN: 8 joins pixels that touch by an edge or a corner, 4 by an edge only
template <int CONN>
__device__ __forceinline__ void merge_step(const CompArgs &a) {
    int n, y, x, rows, cols;
    place(a.p, n, y, x);
    const int h = a.p.h, w = a.p.w;
    if (y >= h || x >= w) return;
    extent_of(a.extent, n, h, w, rows, cols);
    const size_t hw = (size_t)h * w;
    const uint8_t *tg = a.target + (size_t)n * hw;
    const int v = seen(tg, w, rows, cols, a.by_value, y, x);
    if (!v) return;
    int *L = a.labels + (size_t)n * hw;
    const int i = y * w + x;  // < hw <= INT_MAX
    const bool left = seen(tg, w, rows, cols, a.by_value, y, x - 1) == v;
    if (left && (x & 63) == 0) unite(L, i, i - 1);  // the run goes on across the wave seam
    if (y == 0) return;
    const bool up = seen(tg, w, rows, cols, a.by_value, y - 1, x) == v;
    const bool ul = seen(tg, w, rows, cols, a.by_value, y - 1, x - 1) == v;
    if (up) {
        // with left and upper-left in the component, the left pixel joins the two rows
        if (!(left && ul)) unite(L, i, i - w);
    } else if constexpr (CONN == 8) {
        // the left pixel has the upper-left one straight above it, the right pixel the upper-right one
        if (ul && !left) unite(L, i, i - w - 1);
        const bool ur = seen(tg, w, rows, cols, a.by_value, y - 1, x + 1) == v;
        if (ur && seen(tg, w, rows, cols, a.by_value, y, x + 1) != v) unite(L, i, i - w + 1);
    }
}

__global__ __launch_bounds__(kThreads) void obj_merge_kernel(CompArgs a) { merge_step<8>(a); }
__global__ __launch_bounds__(kThreads) void mask_merge4_kernel(CompArgs a) { merge_step<4>(a); }

__global__ __launch_bounds__(kThreads) void obj_flatten_kernel(CompArgs a) {
    int n, y, x;
    place(a.p, n, y, x);
    const int h = a.p.h, w = a.p.w;
    const size_t hw = (size_t)h * w;
    int *L = a.labels + (size_t)n * hw;
    bool root = false;
    if (y < h && x < w) {
        const int i = y * w + x;
        if (load_entry(L + i) != 0) {
            // others' entries may already hold 1 + root: still an ancestor, the walk ends on the same root
            const int r = find_root(L, i);
            root = r == i;
            if (!root) L[i] = r + 1;
        }
    }
    const unsigned long long roots = __ballot(root);
    __shared__ unsigned wave_sum[kThreads / 64];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = (unsigned)__popcll(roots);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int k = 0; k < kThreads / 64; ++k) s += wave_sum[k];
        a.partial[blockIdx.x] = s;  // every block writes its partial
    }
}

// out[n] = sum of the bx partials of image n, in a fixed order (one wave per image)
__global__ __launch_bounds__(64) void obj_total_kernel(const unsigned long long *partial, int bx, long long *out) {
    const int n = blockIdx.x;
    unsigned long long s = 0;
    for (int b = threadIdx.x; b < bx; b += 64) s += partial[(size_t)n * bx + b];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if (threadIdx.x == 0) out[n] = (long long)s;
}

// ---- boxes and cover -------------------------------------------------------------------------------------------
struct CoverArgs {
    const int *labels;
    const int32_t *extent;
    uint16_t *cover;
    int *xmin, *xmax, *ymax;  // [n][hw], used at root pixels only
    uint32_t *diff;           // [n][h][w]: corner differences, then their row sums
    int h, w, bx;
};

// label of (y, x) as the cover sees it: 0 outside plane or extent
__device__ __forceinline__ int label_at(const int *lab, int w, int rows, int cols, int y, int x) {
    return (y < 0 || x < 0 || y >= rows || x >= cols) ? 0 : lab[(size_t)y * w + x];
}

// every root's limits start at the root itself; the difference plane is cleared
__global__ __launch_bounds__(kThreads) void obj_box_init_kernel(CoverArgs a) {
    const int n = blockIdx.x / a.bx;
    const size_t hw = (size_t)a.h * a.w, off = (size_t)n * hw;
    const size_t stride = (size_t)a.bx * kThreads;
    for (size_t i = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; i < hw; i += stride) {
        a.diff[off + i] = 0;
        if (a.labels[off + i] == (int)i + 1) {
            const int x = (int)(i % a.w);
            a.xmin[off + i] = x, a.xmax[off + i] = x, a.ymax[off + i] = (int)(i / a.w);
        }
    }
}

// a pixel at the rim of its component moves the limits kept at the root
__global__ __launch_bounds__(kThreads) void obj_box_kernel(CoverArgs a) {
    const int n = blockIdx.x / a.bx, w = a.w;
    const size_t hw = (size_t)a.h * w, off = (size_t)n * hw;
    const size_t stride = (size_t)a.bx * kThreads;
    int rows, cols;
    extent_of(a.extent, n, a.h, w, rows, cols);
    const int *lab = a.labels + off;
    for (size_t i = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; i < hw; i += stride) {
        const int y = (int)(i / w), x = (int)(i % w);
        const int l = label_at(lab, w, rows, cols, y, x);
        // only a label that names a root pixel (whose limits the first launch set) is used as an index
        if (l < 1 || (size_t)l > hw || lab[l - 1] != l) continue;
        const size_t r = off + (size_t)(l - 1);
        if (label_at(lab, w, rows, cols, y, x - 1) != l) atomicMin(a.xmin + r, x);
        if (label_at(lab, w, rows, cols, y, x + 1) != l) atomicMax(a.xmax + r, x);
        if (label_at(lab, w, rows, cols, y + 1, x) != l) atomicMax(a.ymax + r, y);
    }
}

// one +1 / -1 per corner of every root's box; corners on the far edges (row h, column w) fall outside every sum
__global__ __launch_bounds__(kThreads) void obj_corner_kernel(CoverArgs a) {
    const int n = blockIdx.x / a.bx, w = a.w, h = a.h;
    const size_t hw = (size_t)h * w, off = (size_t)n * hw;
    const size_t stride = (size_t)a.bx * kThreads;
    int rows, cols;
    extent_of(a.extent, n, h, w, rows, cols);
    uint32_t *d = a.diff + off;
    for (size_t i = (size_t)(blockIdx.x % a.bx) * kThreads + threadIdx.x; i < hw; i += stride) {
        if (a.labels[off + i] != (int)i + 1) continue;
        const int ymin = (int)(i / w);  // the root is the first pixel of its component in row-major order
        if (ymin >= rows || (int)(i % w) >= cols) continue;  // a root outside the extent (labels made with another one)
        const int y0 = std::max(0, ymin - 1), y1 = std::min(rows, a.ymax[off + i] + 2);
        const int x0 = std::max(0, a.xmin[off + i] - 1), x1 = std::min(cols, a.xmax[off + i] + 2);
        if (y0 >= y1 || x0 >= x1) continue;  // (cannot happen for a root inside the extent; keeps the adds in bounds)
        // y0 < y1 <= h and x0 < x1 <= w
        atomicAdd(d + (size_t)y0 * w + x0, 1u);
        if (x1 < w) atomicAdd(d + (size_t)y0 * w + x1, ~0u);
        if (y1 < h) atomicAdd(d + (size_t)y1 * w + x0, ~0u);
        if (x1 < w && y1 < h) atomicAdd(d + (size_t)y1 * w + x1, 1u);
    }
}

// in place, one wave per row: diff[y][x] = sum of diff[y][0..x] (modulo 2^32; the cover itself is small)
__global__ __launch_bounds__(kThreads) void obj_rowscan_kernel(CoverArgs a, size_t total_rows) {
    const size_t row = (size_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= total_rows) return;  // whole waves leave
    const int lane = threadIdx.x & 63, w = a.w;
    uint32_t *d = a.diff + row * w;
    uint32_t carry = 0;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        uint32_t v = x < w ? d[x] : 0u;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t o = __shfl_up(v, s, 64);
            if (lane >= s) v += o;
        }
        v += carry;
        if (x < w) d[x] = v;
        carry = __shfl(v, 63, 64);
    }
}

// one lane per column: cover[y][x] = sum of the row sums of rows 0..y
__global__ __launch_bounds__(kThreads) void obj_colscan_kernel(CoverArgs a, size_t total_cols) {
    const size_t col = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (col >= total_cols) return;
    const int w = a.w, h = a.h;
    const size_t off = (col / w) * ((size_t)h * w) + col % w;
    const uint32_t *d = a.diff + off;
    uint16_t *c = a.cover + off;
    uint32_t s = 0;
    int y = 0;
    for (; y + 8 <= h; y += 8) {
        uint32_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = d[(size_t)(y + j) * w];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s += v[j];
            c[(size_t)(y + j) * w] = (uint16_t)s;
        }
    }
    for (; y < h; ++y) {
        s += d[(size_t)y * w];
        c[(size_t)y * w] = (uint16_t)s;
    }
}

// ---- weighted counts -------------------------------------------------------------------------------------------
struct TallyArgs {
    const float *logits;
    const uint8_t *target;
    const uint16_t *cover;
    unsigned long long *partial;  // [n][bx][kPartial]
    size_t hw;
    int c, top_k, bx;
    float t;
};

template <bool MULTI>
__global__ __launch_bounds__(kThreads) void obj_tally_kernel(TallyArgs a) {
    const int n = blockIdx.x / a.bx, tid = threadIdx.x;
    const size_t hw = a.hw, stride = (size_t)a.bx * kThreads;
    const int C = a.c;
    const float *lg = a.logits + (size_t)n * C * hw;
    const uint8_t *tg = a.target + (size_t)n * hw;
    const uint16_t *cv = a.cover + (size_t)n * hw;
    Tally<unsigned long long> ty = {{0, 0, 0, 0}};
    for (size_t p = (size_t)(blockIdx.x % a.bx) * kThreads + tid; p < hw; p += stride) {
        const unsigned long long wgt = cv[p];
        if (!wgt) continue;
        if constexpr (!MULTI) {
            float x = lg[p];
            decide_binary(x, a.t, (int)tg[p], false, wgt, ty);
        } else {
            decide_stream<false>(lg, nullptr, hw, p, C, (int)tg[p], a.top_k, wgt, ty);
            ty.v[2] += wgt;
        }
    }
    block_tally_store<kThreads>(ty, a.partial);
}

// ---- weighted histograms ---------------------------------------------------------------------------------------
struct HistArgs {
    const float *logits;
    const uint8_t *target;
    const uint16_t *cover;
    const int32_t *extent;
    unsigned long long *partial;  // [n][bx][2][B]
    int h, w, bits, bx;
};

__global__ __launch_bounds__(kHistThreads) void obj_hist_kernel(HistArgs a) {
    extern __shared__ uint32_t hist[];  // [2][B]
    const int n = blockIdx.x / a.bx, tid = threadIdx.x;
    const uint32_t B = 1u << a.bits;
    const int shift = 32 - a.bits;
    int rows, cols;
    extent_of(a.extent, n, a.h, a.w, rows, cols);
    const size_t w = (size_t)a.w, hw = (size_t)a.h * w;
    const size_t lim = cols > 0 ? (size_t)rows * w : 0;
    const size_t per_block = (lim + a.bx - 1) / a.bx;
    const size_t p0 = std::min(lim, (size_t)(blockIdx.x % a.bx) * per_block), p1 = std::min(lim, p0 + per_block);
    const float *lg = a.logits + (size_t)n * hw;
    const uint8_t *tg = a.target + (size_t)n * hw;
    const uint16_t *cv = a.cover + (size_t)n * hw;
    unsigned long long *out = a.partial + (size_t)blockIdx.x * 2 * B;
    for (uint32_t i = tid; i < 2 * B; i += kHistThreads) {
        hist[i] = 0;
        out[i] = 0;  // every (image, block) writes its whole partial, work or not
    }
    __syncthreads();
    for (size_t c0 = p0; c0 < p1; c0 += kChunk) {
        const size_t c1 = std::min(p1, c0 + kChunk);  // at most kChunk pixels of at most 65535 each: below 2^32 a word
        for (size_t p = c0 + tid; p < c1; p += kHistThreads) {
            const uint32_t wgt = cv[p];
            if (wgt && (int)(p % w) < cols) atomicAdd(&hist[(tg[p] ? B : 0u) + roc_bin(lg[p], shift)], wgt);
        }
        __syncthreads();
        for (uint32_t i = tid; i < 2 * B; i += kHistThreads) {  // a lane flushes and clears the words it owns
            const uint32_t v = hist[i];
            if (v) {
                out[i] += v;
                hist[i] = 0;
            }
        }
        __syncthreads();
    }
}

// ---- shapes ----------------------------------------------------------------------------------------------------
// wave-per-row-segment placement of the labelling kernels; false if the grid would not fit
bool plane_of(int n, int h, int w, Plane &p) {
    p.h = h, p.w = w, p.wseg = (w + 63) / 64;
    const size_t slots = (size_t)h * p.wseg * 64;
    const size_t bx = (slots + kThreads - 1) / kThreads;
    if (bx * (size_t)n > (size_t)INT_MAX) return false;
    p.bx = (int)bx;
    return true;
}

// blocks per image of the grid-stride kernels
int stride_blocks(int n, size_t hw) { return blocks_for(n, hw, kThreads, kBlocksTarget); }

// blocks per image of the histogram: one per kChunk pixels
int hist_blocks(int n, int h, int w, int bits) {
    return blocks_for(n, (size_t)h * (size_t)w, kChunk, hist_blocks_target(bits));
}

}  // namespace

size_t components_workspace(int n, int h, int w) {
    Plane p;
    if (!plane_ok(n, h, w) || !plane_of(n, h, w, p)) return 0;
    return (size_t)n * p.bx * sizeof(unsigned long long);
}

int launch_components(const uint8_t *target, const int32_t *extent, int n, int h, int w, int mode, int connectivity,
                      int32_t *labels, long long *n_objects, void *workspace, hipStream_t st) {
    CompArgs a;
    if (!plane_of(n, h, w, a.p)) return fail(CAE_ERR_ARG, "%d planes of %d x %d are too many for one call", n, h, w);
    a.target = target, a.extent = extent, a.labels = labels, a.by_value = mode;
    a.partial = static_cast<unsigned long long *>(workspace);
    const dim3 grid((unsigned)((size_t)n * a.p.bx)), block(kThreads);
    hipLaunchKernelGGL(obj_init_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    if (connectivity == 8)
        hipLaunchKernelGGL(obj_merge_kernel, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(mask_merge4_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_flatten_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    if (n_objects) {
        hipLaunchKernelGGL(obj_total_kernel, dim3(n), dim3(64), 0, st, a.partial, a.p.bx, n_objects);
        HIP_TRY(hipGetLastError());
    }
    return CAE_OK;
}

}  // namespace cae

using namespace cae;

extern "C" size_t cae_seg_components_workspace(int n, int h, int w) { return components_workspace(n, h, w); }

extern "C" int cae_seg_components(const uint8_t *target, const int32_t *extent, int n, int h, int w, int by_value,
                                  int32_t *labels, int64_t *n_objects, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_seg_components: bad shape n=%d h=%d w=%d", n, h, w);
    if (!plane_fits(h, w))
        return fail(CAE_ERR_ARG, "cae_seg_components: planes of %d x %d pixels are too large", h, w);
    if (n == 0) return CAE_OK;
    if (!target || !labels || !n_objects) return fail(CAE_ERR_ARG, "cae_seg_components: NULL target, labels or n_objects");
    if (misaligned(labels, 3) || misaligned(n_objects, 7) || (extent && misaligned(extent, 3)))
        return fail(CAE_ERR_ARG, "cae_seg_components: labels / extent not 4-byte or n_objects not 8-byte aligned");
    Plane p;
    if (!plane_of(n, h, w, p)) return fail(CAE_ERR_ARG, "cae_seg_components: %d planes of %d x %d are too many for one call", n, h, w);
    const size_t need = cae_seg_components_workspace(n, h, w);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 7))
        return fail(CAE_ERR_ARG, "cae_seg_components: workspace NULL, not 8-byte aligned or too small: %zu bytes needed", need);
    return launch_components(target, extent, n, h, w, by_value ? kByValue : kAny, 8, labels,
                             reinterpret_cast<long long *>(n_objects), workspace, (hipStream_t)stream);
}

extern "C" size_t cae_seg_object_cover_workspace(int n, int h, int w) {
    if (!plane_ok(n, h, w)) return 0;
    return (size_t)n * (size_t)h * (size_t)w * 4 * sizeof(int32_t);
}

extern "C" int cae_seg_object_cover(const int32_t *labels, const int32_t *extent, int n, int h, int w, uint16_t *cover,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_seg_object_cover: bad shape n=%d h=%d w=%d", n, h, w);
    if (!plane_fits(h, w))
        return fail(CAE_ERR_ARG, "cae_seg_object_cover: planes of %d x %d pixels are too large", h, w);
    if (n == 0) return CAE_OK;
    if (!labels || !cover) return fail(CAE_ERR_ARG, "cae_seg_object_cover: NULL labels or cover");
    if (misaligned(labels, 3) || misaligned(cover, 1) || (extent && misaligned(extent, 3)))
        return fail(CAE_ERR_ARG, "cae_seg_object_cover: labels / extent not 4-byte or cover not 2-byte aligned");
    const size_t need = cae_seg_object_cover_workspace(n, h, w);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 3))
        return fail(CAE_ERR_ARG, "cae_seg_object_cover: workspace NULL, not 4-byte aligned or too small: %zu bytes needed", need);
    const size_t hw = (size_t)h * w, all = (size_t)n * hw;
    const size_t rows = (size_t)n * h, cols = (size_t)n * w;
    const size_t row_blocks = (rows + kThreads / 64 - 1) / (kThreads / 64);
    if (row_blocks > (size_t)INT_MAX) return fail(CAE_ERR_ARG, "cae_seg_object_cover: %d planes of %d x %d are too many for one call", n, h, w);
    CoverArgs a;
    a.labels = labels, a.extent = extent, a.cover = cover;
    a.xmin = static_cast<int *>(workspace), a.xmax = a.xmin + all, a.ymax = a.xmax + all;
    a.diff = reinterpret_cast<uint32_t *>(a.ymax + all);
    a.h = h, a.w = w, a.bx = stride_blocks(n, hw);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((size_t)n * a.bx)), block(kThreads);  // n bx <= max(n, kBlocksTarget)
    hipLaunchKernelGGL(obj_box_init_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_box_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_corner_kernel, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_rowscan_kernel, dim3((unsigned)row_blocks), block, 0, st, a, rows);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(obj_colscan_kernel, dim3((unsigned)((cols + kThreads - 1) / kThreads)), block, 0, st, a, cols);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" size_t cae_seg_object_counts_workspace(int n, int c, size_t hw) {
    if (n < 1 || c < 1 || c > 256 || hw < 1) return 0;
    return (size_t)n * stride_blocks(n, hw) * kPartial * sizeof(unsigned long long);
}

extern "C" int cae_seg_object_counts(const float *logits, const uint8_t *target, const uint16_t *cover, int n, int c,
                                     size_t hw, float t, int top_k, int64_t *counts, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    if (c < 1 || c > 256) return fail(CAE_ERR_ARG, "cae_seg_object_counts: %d classes outside 1..256", c);
    if (n < 0 || hw < 1) return fail(CAE_ERR_ARG, "cae_seg_object_counts: bad shape n=%d hw=%zu", n, hw);
    if (top_k < 1) return fail(CAE_ERR_ARG, "cae_seg_object_counts: top_k %d below 1", top_k);
    if (n == 0) return CAE_OK;
    if (!logits || !target || !cover || !counts)
        return fail(CAE_ERR_ARG, "cae_seg_object_counts: NULL logits, target, cover or counts");
    if (misaligned(logits, 3) || misaligned(cover, 1) || misaligned(counts, 7))
        return fail(CAE_ERR_ARG, "cae_seg_object_counts: logits not 4-byte, cover not 2-byte or counts not 8-byte aligned");
    const size_t need = cae_seg_object_counts_workspace(n, c, hw);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 7))
        return fail(CAE_ERR_ARG, "cae_seg_object_counts: workspace NULL, not 8-byte aligned or too small: %zu bytes needed", need);
    TallyArgs a;
    a.logits = logits, a.target = target, a.cover = cover, a.partial = static_cast<unsigned long long *>(workspace);
    a.hw = hw, a.c = c, a.top_k = std::min(top_k, c), a.bx = stride_blocks(n, hw), a.t = t;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((size_t)n * a.bx)), block(kThreads);
    if (c == 1)
        hipLaunchKernelGGL(obj_tally_kernel<false>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(obj_tally_kernel<true>, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return launch_seg_record(a.partial, n, a.bx, c, -1, reinterpret_cast<long long *>(counts), st);  // -1: total in tally 2
}

extern "C" size_t cae_seg_object_roc_workspace(int n, int h, int w, int bits) {
    if (n < 1 || h < 1 || w < 1 || !bits_ok(bits)) return 0;
    return (size_t)n * hist_blocks(n, h, w, bits) * (sizeof(unsigned long long) << (bits + 1));
}

extern "C" int cae_seg_object_roc_hist(const float *logits, const uint8_t *target, const uint16_t *cover,
                                       const int32_t *extent, int n, int h, int w, int bits, int per_image,
                                       int64_t *hist, void *workspace, size_t workspace_bytes, void *stream) {
    if (!bits_ok(bits)) return refuse_bits("cae_seg_object_roc_hist", bits);
    if (n < 0 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "cae_seg_object_roc_hist: bad shape n=%d h=%d w=%d", n, h, w);
    if (n == 0) return CAE_OK;
    if (!logits || !target || !cover || !hist)
        return fail(CAE_ERR_ARG, "cae_seg_object_roc_hist: NULL logits, target, cover or histogram");
    if (misaligned(logits, 3) || misaligned(cover, 1) || misaligned(hist, 7) || (extent && misaligned(extent, 3)))
        return fail(CAE_ERR_ARG, "cae_seg_object_roc_hist: logits / extent not 4-byte, cover not 2-byte or histogram not 8-byte aligned");
    const size_t need = cae_seg_object_roc_workspace(n, h, w, bits);
    if (!workspace || workspace_bytes < need || misaligned(workspace, 7))
        return fail(CAE_ERR_ARG, "cae_seg_object_roc_hist: workspace NULL, not 8-byte aligned or too small: %zu bytes needed", need);
    HistArgs a;
    a.logits = logits, a.target = target, a.cover = cover, a.extent = extent;
    a.partial = static_cast<unsigned long long *>(workspace);
    a.h = h, a.w = w, a.bits = bits, a.bx = hist_blocks(n, h, w, bits);
    const int lds = (int)(sizeof(uint32_t) << (bits + 1));
    CAE_TRY(ensure_lds(reinterpret_cast<const void *>(obj_hist_kernel), lds));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(obj_hist_kernel, dim3((unsigned)((size_t)n * a.bx)), dim3(kHistThreads), lds, st, a);
    HIP_TRY(hipGetLastError());
    return launch_seg_histsum(a.partial, n, a.bx, per_image, bits, reinterpret_cast<long long *>(hist), st);
}
