// Training input on the device: crop, noise, normalise and rotate patches out of a pool of uint8 HWC tiles in HBM,
// written as the fp32 NCHW batch train_step and the losses take (contract: include/cae_hip.h, cae_t_sample_patches).
//
// Reference: the per-patch CPU transform of utils/datasets/_augs.py:197-264 (get_zarr_transform, label_density == 0):
// ToTensor, AddGaussianNoise(0, 0.001), RandomCrop(pad_if_needed), Normalize(0.5, 0.5), bilinear RandomRotation.  The
// random draws (tile, offsets, angle) stay on the host (sampler.py); the kernels do the per-pixel work.
//
// Both kernels are output-stationary and exchange nothing between lanes: no LDS, no atomics.  The noise of a patch pixel
// is a pure function of (seed, sample index, patch pixel) -- Philox4x32-10, one evaluation gives the normals of all (at most
// four) channels -- so whichever output pixel reads a patch pixel sees the same value, and the result does not depend on
// the launch shape.
//   sample_rows_kernel<C, VEC>   no rotation: a thread takes 4 adjacent pixels of a patch row; inside the image that is
//                                one contiguous 4 C-byte read, and one 16-byte store per channel plane (VEC: ps % 4 == 0
//                                and a 16-byte aligned output; else dword stores with a tail)
//   sample_rotate_kernel<C>      rotation: one output pixel per thread, the four bilinear taps regenerated
//
// Labelled patches (cae_t_sample_labeled_patches; reference: RandomRotationInputTarget, _augs.py:52-82, label_density == 2):
// image and mask share crop and angle; the image is resampled by the exactly interpolating quartic B-spline with reflected
// edges, the mask by its nearest neighbour.  The spline needs the patch's interpolation coefficients first -- a recursive
// filter along every row, then every column -- so these kernels do exchange values between lanes:
//   labeled_lds_kernel<C>        ps <= 128: one block per (sample, channel).  The plane of p is built in LDS (odd row
//                                stride: a lane per row and a lane per column both walk distinct banks), filtered there
//                                along rows then columns (one lane per line), and every output pixel reads its 5 x 5
//                                coefficients from LDS; the block of channel 0 also writes the sample's mask
//   prefilter_global_kernel      ps > 128: p is written to the workspace by sample_rows_kernel, filtered in place (one
//   labeled_global_kernel<C>     lane per line, one launch per axis) and read back from global memory by the evaluation
//   mask_rows_kernel             no rotation: t = m (x is sample_rows_kernel's p)
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"
#include "cae_spline.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

using namespace cae;

namespace {

struct SampleArgs {
    const uint8_t *pool;     // [T][H][W][C]
    const int32_t *tile_hw;  // [T][2] valid rows, columns of each tile, or null (H, W)
    const int32_t *tile, *y0, *x0;
    const float *cosa, *sina;  // null: no rotation
    float *out;                // [n][C][ps][ps]
    int T, H, W, ps;
    uint32_t key0, key1, sample_base;
    float noise_std;
    int normalize;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// -2 ln u for u = (w + 0.5) 2^-32.  In the upper half u = 1 - t with t = (~w + 0.5) 2^-32 exact enough in float32 where
// u itself is not (u rounds to 1 for w >= 2^32 - 128): log1pf keeps the radius of small normals to a few ulp.
__device__ __forceinline__ float neg2_log_u(uint32_t w) {
    const float u = ((float)w + 0.5f) * 0x1p-32f, t = ((float)~w + 0.5f) * 0x1p-32f;
    return -2.0f * ((w & 0x80000000u) ? log1pf(-t) : logf(u));
}

// normals 0, 1 from words 0, 1 and normals 2, 3 from words 2, 3 (Box-Muller: r cos 2 pi u', r sin 2 pi u')
template <int C>
__device__ __forceinline__ void normals(const SampleArgs &a, uint32_t sample, uint32_t pixel, float (&g)[4]) {
    uint32_t r[4];
    philox4x32_10(sample, pixel, 0u, 0u, a.key0, a.key1, r);
    float s, c;
    const float rad0 = sqrtf(neg2_log_u(r[0]));
    sincospif(((float)r[1] + 0.5f) * 0x1p-31f, &s, &c);
    g[0] = rad0 * c;
    g[1] = rad0 * s;
    if (C > 2) {
        const float rad1 = sqrtf(neg2_log_u(r[2]));
        sincospif(((float)r[3] + 0.5f) * 0x1p-31f, &s, &c);
        g[2] = rad1 * c;
        g[3] = rad1 * s;
    } else {
        g[2] = g[3] = 0.0f;
    }
}

// The placement of one sample: its offsets and its tile's valid extent.  Every value is clamped so that no index the
// kernels form can leave the pool or overflow, whatever the device arrays hold: a tile outside [0, T) has no valid pixel.
struct Placement {
    int y0, x0, hv, wv;
};

__device__ __forceinline__ Placement placement(const SampleArgs &a, int s) {
    Placement p;
    const int t = a.tile[s];
    const bool ok = t >= 0 && t < a.T;
    p.hv = ok ? a.H : 0;
    p.wv = ok ? a.W : 0;
    if (ok && a.tile_hw) {
        p.hv = min(max(a.tile_hw[2 * t], 0), a.H);
        p.wv = min(max(a.tile_hw[2 * t + 1], 0), a.W);
    }
    // offsets beyond (-ps, extent) select nothing but padding: clamping them keeps y0 + py inside int
    p.y0 = min(max(a.y0[s], -a.ps), a.H);
    p.x0 = min(max(a.x0[s], -a.ps), a.W);
    return p;
}

template <int C>
__device__ __forceinline__ const uint8_t *tile_base(const SampleArgs &a, int s) {
    const int t = a.tile[s];
    return a.pool + (size_t)((t >= 0 && t < a.T) ? t : 0) * a.H * a.W * C;
}

// v -> p of the contract: u8 / 255 correctly rounded (IEEE division), + noise, clamp, normalise
__device__ __forceinline__ float finish(const SampleArgs &a, uint8_t u8, float g) {
    float v = __fdiv_rn((float)u8, 255.0f);
    if (a.noise_std != 0.0f) v = fminf(fmaxf(v + a.noise_std * g, 0.0f), 1.0f);
    return a.normalize ? (v - 0.5f) / 0.5f : v;
}

// the C values p of patch pixel (py, px), 0 <= py, px < ps
template <int C>
__device__ __forceinline__ void patch_pixel(const SampleArgs &a, const Placement &pl, const uint8_t *img, uint32_t sample,
                                            int py, int px, float (&p)[C]) {
    const int iy = pl.y0 + py, ix = pl.x0 + px;
    if (iy >= 0 && iy < pl.hv && ix >= 0 && ix < pl.wv) {
        float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.noise_std != 0.0f) normals<C>(a, sample, (uint32_t)(py * a.ps + px), g);
        const uint8_t *src = img + ((size_t)iy * a.W + ix) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) p[ch] = finish(a, src[ch], g[ch]);
    } else {
        const float pad = a.normalize ? -1.0f : 0.0f;  // pad_if_needed's zeros, then Normalize
#pragma unroll
        for (int ch = 0; ch < C; ++ch) p[ch] = pad;
    }
}

template <int C, bool VEC>
__global__ void __launch_bounds__(256) sample_rows_kernel(const SampleArgs a, int strips) {
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int groups = (a.ps + 3) >> 2;
    const int item = strip * 256 + threadIdx.x;
    if (item >= a.ps * groups) return;
    const int py = item / groups, px = (item - py * groups) * 4;
    const Placement pl = placement(a, s);
    const uint8_t *img = tile_base<C>(a, s);
    const uint32_t sample = a.sample_base + (uint32_t)s;
    float p[4][C];
    const int iy = pl.y0 + py, ix = pl.x0 + px;
    if (iy >= 0 && iy < pl.hv && ix >= 0 && ix + 3 < pl.wv && px + 3 < a.ps) {
        uint8_t raw[4 * C];
        __builtin_memcpy(raw, img + ((size_t)iy * a.W + ix) * C, 4 * C);  // one contiguous read, any alignment
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.noise_std != 0.0f) normals<C>(a, sample, (uint32_t)(py * a.ps + px + k), g);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) p[k][ch] = finish(a, raw[k * C + ch], g[ch]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (px + k < a.ps) patch_pixel<C>(a, pl, img, sample, py, px + k, p[k]);
    }
    float *o = a.out + ((size_t)s * C * a.ps + py) * a.ps + px;
    const size_t plane = (size_t)a.ps * a.ps;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        if (VEC) {
            *reinterpret_cast<float4 *>(o + ch * plane) = make_float4(p[0][ch], p[1][ch], p[2][ch], p[3][ch]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (px + k < a.ps) o[ch * plane + k] = p[k][ch];
        }
    }
}

template <int C>
__global__ void __launch_bounds__(256) sample_rotate_kernel(const SampleArgs a, int strips) {
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int item = strip * 256 + threadIdx.x;
    if (item >= a.ps * a.ps) return;
    const int i = item / a.ps, j = item - i * a.ps;
    const Placement pl = placement(a, s);
    const uint8_t *img = tile_base<C>(a, s);
    const uint32_t sample = a.sample_base + (uint32_t)s;
    const float ca = a.cosa[s], sa = a.sina[s];
    const float c = 0.5f * (float)(a.ps - 1), dx = (float)j - c, dy = (float)i - c;
    const float sx = c + (ca * dx - sa * dy), sy = c + (sa * dx + ca * dy);
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
    // a source point outside (-1, ps) has no tap inside the patch (this also keeps NaN / huge coordinates out of the casts)
    if (sx > -1.0f && sx < (float)a.ps && sy > -1.0f && sy < (float)a.ps) {
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const int tx0 = (int)fx0, ty0 = (int)fy0;
        const float wx1 = sx - fx0, wy1 = sy - fy0, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ty = ty0 + (t >> 1), tx = tx0 + (t & 1);
            if (ty < 0 || ty >= a.ps || tx < 0 || tx >= a.ps) continue;  // zero fill
            const float w = ((t >> 1) ? wy1 : wy0) * ((t & 1) ? wx1 : wx0);
            float p[C];
            patch_pixel<C>(a, pl, img, sample, ty, tx, p);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] += w * p[ch];
        }
    }
    float *o = a.out + (size_t)s * C * a.ps * a.ps + item;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[(size_t)ch * a.ps * a.ps] = acc[ch];
}

template <int C>
void launch(const SampleArgs &a, int n, bool vec, hipStream_t st) {
    if (a.cosa) {
        const int strips = (a.ps * a.ps + 255) / 256;
        hipLaunchKernelGGL(sample_rotate_kernel<C>, dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
    } else {
        const int strips = (a.ps * ((a.ps + 3) / 4) + 255) / 256;
        if (vec)
            hipLaunchKernelGGL((sample_rows_kernel<C, true>), dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
        else
            hipLaunchKernelGGL((sample_rows_kernel<C, false>), dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
    }
}

// ---- labelled patches: quartic B-spline rotation of the image, nearest neighbour of the mask ----------------------------

struct LabeledArgs {
    SampleArgs s;           // the image side; s.out is x
    const uint8_t *labels;  // [T][H][W][K]
    float *t;               // [n][Kt][ps][ps], Kt = map_labels ? 1 : K
    float *coef;            // the workspace, [n][C][ps][ps] (ps > LDS_PS only)
    int K, map_labels;
};

constexpr int LDS_PS = 128;  // the largest patch whose plane is filtered and sampled in LDS

// The poles of the quartic B-spline's inverse filter, sqrt(664 -+ sqrt(438976)) +- sqrt(304) - 19, and the gain of a line,
// the product over both of (1 - z)(1 - 1 / z) = 384 (the samples of the spline are 1, 76, 230, 76, 1 over 384).
constexpr float POLE1 = -0.36134122590021184f, POLE2 = -0.013725429297341663f;
constexpr float SPLINE_GAIN = 384.0f;
// The start of the causal recursion sums z^i over the whole line.  |POLE1|^28 < 2^-41: the terms from 28 on change no
// float32 sum, and z^n is below 2^-93 from n = 64 on (the line's other end reaches the start with that weight).
constexpr int START_TERMS = 28, POWER_TERMS = 64;

// (the recursion over one pole and `reflect` live in cae_spline.hpp, shared with the cubic spline of cae_elastic.hip)
__device__ __forceinline__ void filter_line(float *c, int n, int stride) {
    filter_pole<START_TERMS, POWER_TERMS>(c, n, stride, POLE1, SPLINE_GAIN);
    filter_pole<START_TERMS, POWER_TERMS>(c, n, stride, POLE2, 1.0f);
}

// the quartic B-spline at distance d; 0 from 2.5 on
__device__ __forceinline__ float bspline4(float d) {
    d = fabsf(d);
    if (d < 0.5f) return d * d * (d * d * 0.25f - 0.625f) + 115.0f / 192.0f;
    if (d < 1.5f) return d * (d * (d * (5.0f / 6.0f - d * (1.0f / 6.0f)) - 1.25f) + 5.0f / 24.0f) + 55.0f / 96.0f;
    const float e = fminf(d, 2.5f) - 2.5f;
    return e * e * e * e * (1.0f / 24.0f);
}

// what output pixel (i, j) reads: five reflected rows and columns with their weights; the mask's nearest neighbour is the
// middle tap
struct Taps {
    int ry[5], rx[5];
    float wy[5], wx[5];
};

__device__ __forceinline__ void taps_of(int ps, float ca, float sa, int i, int j, Taps &t) {
    const float c = 0.5f * (float)(ps - 1), di = (float)i - c, dj = (float)j - c;
    // |cos|, |sin| <= 1 keep a source point within (-0.21 ps, 1.21 ps).  Whatever else the device arrays hold is clamped
    // to [-ps, 2 ps] before the cast (fmaxf returns the bound for a NaN), so the tap indices stay within a few ps.
    const float lo = -(float)ps, hi = 2.0f * (float)ps;
    const float y = fminf(fmaxf(c + (ca * di + sa * dj), lo), hi);
    const float x = fminf(fmaxf(c + (ca * dj - sa * di), lo), hi);
    const int ny = (int)floorf(y + 0.5f), nx = (int)floorf(x + 0.5f);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int ty = ny - 2 + k, tx = nx - 2 + k;
        t.ry[k] = reflect(ty, ps);
        t.rx[k] = reflect(tx, ps);
        t.wy[k] = bspline4(y - (float)ty);
        t.wx[k] = bspline4(x - (float)tx);
    }
}

// the 25 taps over coefficients c[row * stride + column]
__device__ __forceinline__ float spline_at(const float *c, int stride, const Taps &t) {
    float acc = 0.0f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const float *row = c + t.ry[a] * stride;
        float r = 0.0f;
#pragma unroll
        for (int b = 0; b < 5; ++b) r += t.wx[b] * row[t.rx[b]];
        acc += t.wy[a] * r;
    }
    return acc;
}

// t of output pixel `item` of sample s: m at patch pixel (my, mx), 0 outside the tile's valid extent
__device__ __forceinline__ void write_mask(const LabeledArgs &a, const Placement &pl, int s, int my, int mx, int item) {
    const SampleArgs &g = a.s;
    const int iy = pl.y0 + my, ix = pl.x0 + mx;
    const bool inside = iy >= 0 && iy < pl.hv && ix >= 0 && ix < pl.wv;
    const int tl = g.tile[s];
    const size_t tile = (tl >= 0 && tl < g.T) ? tl : 0;
    const uint8_t *src = a.labels + ((tile * g.H + (inside ? iy : 0)) * g.W + (inside ? ix : 0)) * a.K;
    const size_t plane = (size_t)g.ps * g.ps;
    float *o = a.t + (size_t)s * (a.map_labels ? 1 : a.K) * plane + item;
    float sum = 0.0f;
    for (int k = 0; k < a.K; ++k) {
        const float v = inside ? (float)src[k] : 0.0f;
        if (a.map_labels)
            sum += v;
        else
            o[k * plane] = v;
    }
    if (a.map_labels) o[0] = sum;
}

template <int C>
__global__ void __launch_bounds__(256) labeled_lds_kernel(const LabeledArgs a) {
    extern __shared__ float plane[];  // [ps][ps | 1]
    const SampleArgs &g = a.s;
    const int s = blockIdx.x / C, ch = blockIdx.x - s * C;
    const int ps = g.ps, stride = ps | 1, tid = threadIdx.x;
    const Placement pl = placement(g, s);
    const uint8_t *img = tile_base<C>(g, s);
    const uint32_t sample = g.sample_base + (uint32_t)s;
    for (int item = tid; item < ps * ps; item += 256) {
        const int py = item / ps, px = item - py * ps;
        float p[C];
        patch_pixel<C>(g, pl, img, sample, py, px, p);
        float v = p[0];
#pragma unroll
        for (int k = 1; k < C; ++k) v = ch == k ? p[k] : v;
        plane[py * stride + px] = v;
    }
    __syncthreads();
    if (tid < ps) filter_line(plane + tid * stride, ps, 1);
    __syncthreads();
    if (tid < ps) filter_line(plane + tid, ps, stride);
    __syncthreads();
    const float ca = g.cosa[s], sa = g.sina[s];
    float *x = g.out + ((size_t)s * C + ch) * ps * ps;
    for (int item = tid; item < ps * ps; item += 256) {
        const int i = item / ps, j = item - i * ps;
        Taps t;
        taps_of(ps, ca, sa, i, j, t);
        x[item] = spline_at(plane, stride, t);
        if (ch == 0) write_mask(a, pl, s, t.ry[2], t.rx[2], item);
    }
}

// one lane per line of the workspace's planes: rows (columns = 0), then columns in a second launch
__global__ void __launch_bounds__(64) prefilter_global_kernel(float *coef, long lines, int ps, int columns) {
    const long line = (long)blockIdx.x * 64 + threadIdx.x;
    if (line >= lines) return;
    const long plane = line / ps;
    const int l = (int)(line - plane * ps);
    filter_line(coef + (size_t)plane * ps * ps + (columns ? (size_t)l : (size_t)l * ps), ps, columns ? ps : 1);
}

template <int C>
__global__ void __launch_bounds__(256) labeled_global_kernel(const LabeledArgs a, int strips) {
    const SampleArgs &g = a.s;
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int ps = g.ps, item = strip * 256 + threadIdx.x;
    if (item >= ps * ps) return;
    const int i = item / ps, j = item - i * ps;
    Taps t;
    taps_of(ps, g.cosa[s], g.sina[s], i, j, t);
    const size_t plane = (size_t)ps * ps;
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        g.out[((size_t)s * C + ch) * plane + item] = spline_at(a.coef + ((size_t)s * C + ch) * plane, ps, t);
    write_mask(a, placement(g, s), s, t.ry[2], t.rx[2], item);
}

__global__ void __launch_bounds__(256) mask_rows_kernel(const LabeledArgs a, int strips) {
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int ps = a.s.ps, item = strip * 256 + threadIdx.x;
    if (item >= ps * ps) return;
    write_mask(a, placement(a.s, s), s, item / ps, item % ps, item);
}

template <int C>
int launch_labeled(const LabeledArgs &a, int n, hipStream_t st) {
    const int ps = a.s.ps, strips = (ps * ps + 255) / 256;
    if (!a.s.cosa) {  // x = p, t = m
        launch<C>(a.s, n, ps % 4 == 0 && ((uintptr_t)a.s.out & 15u) == 0, st);
        hipLaunchKernelGGL(mask_rows_kernel, dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
    } else if (ps <= LDS_PS) {
        const int lds = ps * (ps | 1) * (int)sizeof(float);
        CAE_TRY(ensure_lds((const void *)labeled_lds_kernel<C>, lds));
        hipLaunchKernelGGL(labeled_lds_kernel<C>, dim3((unsigned)(n * C)), dim3(256), (size_t)lds, st, a);
    } else {
        SampleArgs fill = a.s;  // p into the workspace
        fill.cosa = fill.sina = nullptr;
        fill.out = a.coef;
        launch<C>(fill, n, ps % 4 == 0 && ((uintptr_t)a.coef & 15u) == 0, st);
        const long lines = (long)n * C * ps;
        for (int columns = 0; columns < 2; ++columns)
            hipLaunchKernelGGL(prefilter_global_kernel, dim3((unsigned)((lines + 63) / 64)), dim3(64), 0, st, a.coef, lines, ps,
                               columns);
        hipLaunchKernelGGL(labeled_global_kernel<C>, dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
    }
    return CAE_OK;
}

// the argument checks both entry points share; `out` is the image output
int check_sample_args(const void *pool_dev, int tiles, int h, int w, int c, const int32_t *tile_dev, const int32_t *y0_dev,
                      const int32_t *x0_dev, const int32_t *tile_host, const float *cos_dev, const float *sin_dev,
                      float noise_std, int n, int ps, const void *out_dev) {
    if (c < 1 || c > 4) return fail(CAE_ERR_ARG, "1 to 4 channels per pixel, got %d", c);
    if (ps < 1 || ps > 16384) return fail(CAE_ERR_ARG, "patch size %d outside 1 .. 16384", ps);
    if (n < 0) return fail(CAE_ERR_ARG, "n = %d", n);
    if (tiles < 1 || h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24))
        return fail(CAE_ERR_ARG, "pool of %d tiles of %d x %d", tiles, h, w);
    if (!pool_dev || !tile_dev || !y0_dev || !x0_dev || !out_dev) return fail(CAE_ERR_ARG, "NULL argument");
    if ((cos_dev == nullptr) != (sin_dev == nullptr)) return fail(CAE_ERR_ARG, "cos and sin come together");
    if (!(noise_std >= 0.0f) || !(noise_std < 1e30f)) return fail(CAE_ERR_ARG, "noise_std must be finite and >= 0");
    if (tile_host)
        for (int s = 0; s < n; ++s)
            if (tile_host[s] < 0 || tile_host[s] >= tiles)
                return fail(CAE_ERR_ARG, "sample %d names tile %d of %d", s, tile_host[s], tiles);
    const long strips = cos_dev ? ((long)ps * ps + 255) / 256 : ((long)ps * ((ps + 3) / 4) + 255) / 256;
    if ((long)n * strips > 0x7fffffffL) return fail(CAE_ERR_ARG, "%d patches of %d^2 in one call: split the batch", n, ps);
    return CAE_OK;
}

SampleArgs sample_args(const uint8_t *pool_dev, int tiles, int h, int w, const int32_t *tile_hw_dev, const int32_t *tile_dev,
                       const int32_t *y0_dev, const int32_t *x0_dev, const float *cos_dev, const float *sin_dev,
                       uint64_t seed, uint32_t sample_base, float noise_std, int normalize, int ps, float *out_dev) {
    SampleArgs a{};
    a.pool = pool_dev;
    a.tile_hw = tile_hw_dev;
    a.tile = tile_dev, a.y0 = y0_dev, a.x0 = x0_dev;
    a.cosa = cos_dev, a.sina = sin_dev;
    a.out = out_dev;
    a.T = tiles, a.H = h, a.W = w, a.ps = ps;
    a.key0 = (uint32_t)seed, a.key1 = (uint32_t)(seed >> 32), a.sample_base = sample_base;
    a.noise_std = noise_std;
    a.normalize = normalize != 0;
    return a;
}

}  // namespace

extern "C" int cae_t_sample_patches(const uint8_t *pool_dev, int tiles, int h, int w, int c, const int32_t *tile_hw_dev,
                                    const int32_t *tile_dev, const int32_t *y0_dev, const int32_t *x0_dev,
                                    const int32_t *tile_host, const float *cos_dev, const float *sin_dev, uint64_t seed,
                                    uint32_t sample_base, float noise_std, int normalize, int n, int ps, float *out_dev,
                                    void *stream) {
    CAE_TRY(check_sample_args(pool_dev, tiles, h, w, c, tile_dev, y0_dev, x0_dev, tile_host, cos_dev, sin_dev, noise_std, n,
                              ps, out_dev));
    if (n == 0) return CAE_OK;
    const SampleArgs a = sample_args(pool_dev, tiles, h, w, tile_hw_dev, tile_dev, y0_dev, x0_dev, cos_dev, sin_dev, seed,
                                     sample_base, noise_std, normalize, ps, out_dev);
    const bool vec = ps % 4 == 0 && ((uintptr_t)out_dev & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    switch (c) {
        case 1: launch<1>(a, n, vec, st); break;
        case 2: launch<2>(a, n, vec, st); break;
        case 3: launch<3>(a, n, vec, st); break;
        default: launch<4>(a, n, vec, st); break;
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

extern "C" int cae_t_sample_labeled_patches(const uint8_t *pool_dev, const uint8_t *labels_dev, int tiles, int h, int w, int c,
                                            int k, const int32_t *tile_hw_dev, const int32_t *tile_dev,
                                            const int32_t *y0_dev, const int32_t *x0_dev, const int32_t *tile_host,
                                            const float *cos_dev, const float *sin_dev, uint64_t seed, uint32_t sample_base,
                                            float noise_std, int normalize, int map_labels, int n, int ps,
                                            void *workspace_dev, size_t workspace_bytes, float *x_dev, float *t_dev,
                                            void *stream) {
    if (k < 1 || k > 4) return fail(CAE_ERR_ARG, "1 to 4 label channels per pixel, got %d", k);
    if (!labels_dev || !t_dev) return fail(CAE_ERR_ARG, "NULL argument");
    CAE_TRY(check_sample_args(pool_dev, tiles, h, w, c, tile_dev, y0_dev, x0_dev, tile_host, cos_dev, sin_dev, noise_std, n,
                              ps, x_dev));
    // grids: n strips of 256 pixels (mask, global evaluation), n c planes, n c ps lines in blocks of 64
    if ((long)n * (((long)ps * ps + 255) / 256) > 0x7fffffffL || (long)n * c > 0x7fffffffL ||
        (long)n * c * ps > 0x7fffffffL * 64)
        return fail(CAE_ERR_ARG, "%d patches of %d^2 in one call: split the batch", n, ps);
    const size_t need = cos_dev && ps > LDS_PS ? (size_t)n * c * ps * ps * sizeof(float) : 0;
    if (need && (!workspace_dev || workspace_bytes < need))
        return fail(CAE_ERR_ARG, "the workspace holds %zu bytes, %d patches of %d x %d^2 need %zu",
                    workspace_dev ? workspace_bytes : (size_t)0, n, c, ps, need);
    if (n == 0) return CAE_OK;
    LabeledArgs a{};
    a.s = sample_args(pool_dev, tiles, h, w, tile_hw_dev, tile_dev, y0_dev, x0_dev, cos_dev, sin_dev, seed, sample_base,
                      noise_std, normalize, ps, x_dev);
    a.labels = labels_dev;
    a.t = t_dev;
    a.coef = (float *)workspace_dev;
    a.K = k, a.map_labels = map_labels != 0;
    hipStream_t st = (hipStream_t)stream;
    switch (c) {
        case 1: CAE_TRY(launch_labeled<1>(a, n, st)); break;
        case 2: CAE_TRY(launch_labeled<2>(a, n, st)); break;
        case 3: CAE_TRY(launch_labeled<3>(a, n, st)); break;
        default: CAE_TRY(launch_labeled<4>(a, n, st)); break;
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
