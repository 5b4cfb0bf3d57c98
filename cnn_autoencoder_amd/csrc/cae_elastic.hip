// Elastic deformation of a batch of image (and mask) patches that already lies in HBM (contract: include/cae_hip.h,
// cae_t_elastic_deform).
//
// Reference: RandomElasticDeformationInput / RandomElasticDeformationInputTarget of utils/datasets/_augs.py:26-49, 85-99
// (get_zarr_transform with elastic_deformation=True): a 3 x 3 grid of random displacements, interpolated by a cubic
// B-spline to a per-pixel field; the image is resampled through the exactly interpolating cubic B-spline, the mask by its
// nearest neighbour, both with reflected edges.  The nine displacements per axis are the caller's draw; it hands their
// spline coefficients over (float64 on the host, rounded once), the kernels do the per-pixel work.
//
//   elastic_lds_kernel         ps <= 128: one block per (sample, channel) plane.  The plane is loaded into LDS (row stride
//                              ps | 1 dwords: a lane per row and a lane per column both walk distinct banks), filtered there
//                              along rows then columns (one lane per line), and every output pixel reads its 4 x 4
//                              coefficients from LDS.  The folded field weights W_a(u_i) of the ps rows (= columns) are a
//                              table of 3 ps floats behind the plane.  The block of channel 0 also writes the mask planes.
//   prefilter_rows_kernel      ps > 128: a block stages a strip of rows of one plane in LDS (coalesced loads, same odd row
//                              stride), a lane per row filters it there, and the strip goes to the workspace coalesced;
//   prefilter_columns_kernel   the same for a strip of adjacent columns of the workspace, in place: whole columns in LDS
//                              (row stride = the strip's width: the lanes of one row sit on consecutive banks), a lane per
//                              column.  Either way the serial recursion waits on LDS, not on memory;
//   elastic_global_kernel<C>   one output pixel per thread with all C channels: the field is evaluated once per pixel, the
//                              16 taps per channel come from the workspace, and the thread writes the pixel's mask values.
//
// Terms dropped from the start of the recursion (both below float32 resolution for the pole sqrt(3) - 2 = -0.268):
// z^i from i = 22 on (|z|^22 < 2^-41), and z^n from n = 64 on (|z|^64 < 2^-121).
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"
#include "cae_spline.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

using namespace cae;

namespace {

struct ElasticArgs {
    const float *x_in, *t_in;  // [n][c][ps][ps], [n][kt][ps][ps] (null with kt == 0)
    const float *coef;         // [n][2][3][3]
    float *x_out, *t_out;
    float *ws;                 // [n][c][ps][ps]: the interpolation coefficients (ps > LDS_PS only)
    int c, kt, ps;
    float scale;               // 2 / (ps - 1), the grid coordinate of one pixel step (0 with ps == 1)
};

constexpr int LDS_PS = 128;      // the largest patch whose plane is filtered and sampled in LDS
constexpr int STRIP_ROWS = 16;   // rows a block of prefilter_rows_kernel stages, where they fit STRIP_LDS
constexpr int STRIP_COLS = 32;   // columns a block of prefilter_columns_kernel stages, where they fit STRIP_LDS
constexpr int STRIP_LDS = 128 * 1024;
constexpr float POLE = -0.2679491924311227f;  // sqrt(3) - 2; the line's gain (1 - z)(1 - 1 / z) is 6
constexpr float SPLINE_GAIN = 6.0f;
constexpr int START_TERMS = 22, POWER_TERMS = 64;

__device__ __forceinline__ void filter_line(float *c, int n, int stride) {
    filter_pole<START_TERMS, POWER_TERMS>(c, n, stride, POLE, SPLINE_GAIN);
}

// the cubic B-spline at distance d; 0 from 2 on
__device__ __forceinline__ float bspline3(float d) {
    d = fabsf(d);
    if (d < 1.0f) return d * d * (0.5f * d - 1.0f) + 2.0f / 3.0f;
    const float e = 2.0f - fminf(d, 2.0f);
    return e * e * e * (1.0f / 6.0f);
}

// the weights of the three control points of one axis at grid coordinate u in [0, 2]: the mirror extension of the grid
// (... 2 1 | 0 1 2 | 1 0 ...) folded onto them
__device__ __forceinline__ void field_weights(float u, float (&w)[3]) {
    w[0] = bspline3(u);
    w[1] = bspline3(u - 1.0f) + bspline3(u + 1.0f) + bspline3(u - 3.0f);
    w[2] = bspline3(u - 2.0f);
}

// what output pixel (i, j) reads: four reflected rows and columns with their weights, and the mask's nearest neighbour
struct Source {
    int ry[4], rx[4], my, mx;
    float wy[4], wx[4];
};

// cf: the sample's 18 field coefficients; wi, wj: the field weights of row i and column j
__device__ __forceinline__ void source_of(int ps, const float (&cf)[18], const float (&wi)[3], const float (&wj)[3], int i,
                                          int j, Source &s) {
    float d[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float acc = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float r = 0.0f;
#pragma unroll
            for (int b = 0; b < 3; ++b) r += wj[b] * cf[k * 9 + a * 3 + b];
            acc += wi[a] * r;
        }
        d[k] = acc;
    }
    // Whatever the coefficients hold, the source point is clamped to [-ps, 2 ps] before any cast (fmaxf returns the
    // bound for a NaN), so the tap indices stay within a few ps.
    const float lo = -(float)ps, hi = 2.0f * (float)ps;
    const float y = fminf(fmaxf((float)i + d[0], lo), hi);
    const float x = fminf(fmaxf((float)j + d[1], lo), hi);
    s.my = reflect((int)floorf(y + 0.5f), ps);
    s.mx = reflect((int)floorf(x + 0.5f), ps);
    const int ys = (int)floorf(y) - 1, xs = (int)floorf(x) - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s.ry[k] = reflect(ys + k, ps);
        s.rx[k] = reflect(xs + k, ps);
        s.wy[k] = bspline3(y - (float)(ys + k));
        s.wx[k] = bspline3(x - (float)(xs + k));
    }
}

// the 16 taps over coefficients c[row * stride + column]
__device__ __forceinline__ float spline_at(const float *c, int stride, const Source &s) {
    float acc = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float *row = c + (size_t)s.ry[a] * stride;
        float r = 0.0f;
#pragma unroll
        for (int b = 0; b < 4; ++b) r += s.wx[b] * row[s.rx[b]];
        acc += s.wy[a] * r;
    }
    return acc;
}

// the kt mask values of output pixel `item` of sample s: exact copies
__device__ __forceinline__ void write_mask(const ElasticArgs &a, int s, const Source &src, int item) {
    const size_t plane = (size_t)a.ps * a.ps;
    for (int k = 0; k < a.kt; ++k) {
        const size_t base = ((size_t)s * a.kt + k) * plane;
        a.t_out[base + item] = a.t_in[base + (size_t)src.my * a.ps + src.mx];
    }
}

__global__ void __launch_bounds__(256) elastic_lds_kernel(const ElasticArgs a) {
    extern __shared__ float lds[];  // the plane [ps][ps | 1], then the field weights [3][ps]
    const int ps = a.ps, stride = ps | 1, tid = threadIdx.x;
    const int s = blockIdx.x / a.c, ch = blockIdx.x - s * a.c;
    float *plane = lds, *fw = lds + ps * stride;
    const float *in = a.x_in + (size_t)blockIdx.x * ps * ps;
    for (int item = tid; item < ps * ps; item += 256) {
        const int py = item / ps, px = item - py * ps;
        plane[py * stride + px] = in[item];
    }
    for (int i = tid; i < ps; i += 256) {
        float w[3];
        field_weights((float)i * a.scale, w);
        fw[i] = w[0], fw[ps + i] = w[1], fw[2 * ps + i] = w[2];
    }
    __syncthreads();
    if (tid < ps) filter_line(plane + tid * stride, ps, 1);
    __syncthreads();
    if (tid < ps) filter_line(plane + tid, ps, stride);
    __syncthreads();
    float cf[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) cf[q] = a.coef[(size_t)s * 18 + q];
    float *out = a.x_out + (size_t)blockIdx.x * ps * ps;
    for (int item = tid; item < ps * ps; item += 256) {
        const int i = item / ps, j = item - i * ps;
        const float wi[3] = {fw[i], fw[ps + i], fw[2 * ps + i]}, wj[3] = {fw[j], fw[ps + j], fw[2 * ps + j]};
        Source src;
        source_of(ps, cf, wi, wj, i, j, src);
        out[item] = spline_at(plane, stride, src);
        if (ch == 0) write_mask(a, s, src, item);
    }
}

// rows r0 .. r0 + rows of one plane per block: in -> LDS -> filtered -> out
__global__ void __launch_bounds__(256) prefilter_rows_kernel(const float *in, float *out, int ps, int rows, int strips) {
    extern __shared__ float lds[];  // [rows][ps | 1]
    const int plane = blockIdx.x / strips, strip = blockIdx.x - plane * strips;
    const int r0 = strip * rows, nr = min(rows, ps - r0), stride = ps | 1, tid = threadIdx.x;
    const size_t base = ((size_t)plane * ps + r0) * ps;
    for (int item = tid; item < nr * ps; item += 256) {
        const int r = item / ps, col = item - r * ps;
        lds[r * stride + col] = in[base + item];
    }
    __syncthreads();
    if (tid < nr) filter_line(lds + tid * stride, ps, 1);
    __syncthreads();
    for (int item = tid; item < nr * ps; item += 256) {
        const int r = item / ps, col = item - r * ps;
        out[base + item] = lds[r * stride + col];
    }
}

// columns c0 .. c0 + cols of one plane per block, in place: workspace -> LDS -> filtered -> workspace
__global__ void __launch_bounds__(256) prefilter_columns_kernel(float *coef, int ps, int cols, int strips) {
    extern __shared__ float lds[];  // [ps][cols]
    const int plane = blockIdx.x / strips, strip = blockIdx.x - plane * strips;
    const int c0 = strip * cols, nc = min(cols, ps - c0), tid = threadIdx.x;
    float *base = coef + (size_t)plane * ps * ps + c0;
    for (int item = tid; item < ps * nc; item += 256) {
        const int r = item / nc, col = item - r * nc;
        lds[r * cols + col] = base[(size_t)r * ps + col];
    }
    __syncthreads();
    if (tid < nc) filter_line(lds + tid, ps, cols);
    __syncthreads();
    for (int item = tid; item < ps * nc; item += 256) {
        const int r = item / nc, col = item - r * nc;
        base[(size_t)r * ps + col] = lds[r * cols + col];
    }
}

template <int C>
__global__ void __launch_bounds__(256) elastic_global_kernel(const ElasticArgs a, int strips) {
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int ps = a.ps, item = strip * 256 + threadIdx.x;
    if (item >= ps * ps) return;
    const int i = item / ps, j = item - i * ps;
    float cf[18], wi[3], wj[3];
#pragma unroll
    for (int q = 0; q < 18; ++q) cf[q] = a.coef[(size_t)s * 18 + q];
    field_weights((float)i * a.scale, wi);
    field_weights((float)j * a.scale, wj);
    Source src;
    source_of(ps, cf, wi, wj, i, j, src);
    const size_t plane = (size_t)ps * ps;
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        a.x_out[((size_t)s * C + ch) * plane + item] = spline_at(a.ws + ((size_t)s * C + ch) * plane, ps, src);
    write_mask(a, s, src, item);
}

int strip_rows(int ps) { return std::max(1, std::min(STRIP_ROWS, STRIP_LDS / ((ps | 1) * (int)sizeof(float)))); }
int strip_cols(int ps) { return std::max(1, std::min(STRIP_COLS, STRIP_LDS / (ps * (int)sizeof(float)))); }

size_t workspace_need(int n, int c, int ps) { return ps > LDS_PS ? (size_t)n * c * ps * ps * sizeof(float) : 0; }

template <int C>
void launch_global(const ElasticArgs &a, int n, int strips, hipStream_t st) {
    hipLaunchKernelGGL(elastic_global_kernel<C>, dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
}

}  // namespace

extern "C" size_t cae_t_elastic_deform_workspace(int n, int c, int ps) {
    if (n < 0 || c < 1 || c > 4 || ps < 1 || ps > 16384) return 0;
    return workspace_need(n, c, ps);
}

extern "C" int cae_t_elastic_deform(const float *x_in, const float *t_in, const float *coef_dev, int n, int c, int kt, int ps,
                                    void *workspace_dev, size_t workspace_bytes, float *x_out, float *t_out, void *stream) {
    if (c < 1 || c > 4) return fail(CAE_ERR_ARG, "1 to 4 channels per pixel, got %d", c);
    if (kt < 0 || kt > 4) return fail(CAE_ERR_ARG, "0 to 4 mask channels per pixel, got %d", kt);
    if (ps < 1 || ps > 16384) return fail(CAE_ERR_ARG, "patch size %d outside 1 .. 16384", ps);
    if (n < 0) return fail(CAE_ERR_ARG, "n = %d", n);
    if (!x_in || !x_out || !coef_dev) return fail(CAE_ERR_ARG, "NULL argument");
    if (kt > 0 && (!t_in || !t_out)) return fail(CAE_ERR_ARG, "NULL mask argument with %d mask channels", kt);
    if (kt == 0 && (t_in || t_out)) return fail(CAE_ERR_ARG, "a mask argument without mask channels");
    if (x_out == x_in || (kt > 0 && (t_out == t_in || (const float *)t_out == x_in || (const float *)x_out == t_in)))
        return fail(CAE_ERR_ARG, "an output is also an input: the transform does not work in place");
    const size_t need = workspace_need(n, c, ps);
    if (need && (!workspace_dev || workspace_bytes < need))
        return fail(CAE_ERR_ARG, "the workspace holds %zu bytes, %d patches of %d x %d^2 need %zu",
                    workspace_dev ? workspace_bytes : (size_t)0, n, c, ps, need);
    // grids: n c planes (LDS kernel); n c strips of rows, n c strips of columns, n strips of 256 pixels
    const int rows = strip_rows(ps), cols = strip_cols(ps);
    const long row_strips = (ps + rows - 1) / rows, col_strips = (ps + cols - 1) / cols, strips = ((long)ps * ps + 255) / 256;
    const long blocks = ps <= LDS_PS ? (long)n * c : std::max((long)n * c * std::max(row_strips, col_strips), (long)n * strips);
    if (blocks > 0x7fffffffL) return fail(CAE_ERR_ARG, "%d patches of %d x %d^2 in one call: split the batch", n, c, ps);
    if (n == 0) return CAE_OK;
    ElasticArgs a{};
    a.x_in = x_in, a.t_in = t_in, a.coef = coef_dev;
    a.x_out = x_out, a.t_out = t_out;
    a.ws = (float *)workspace_dev;
    a.c = c, a.kt = kt, a.ps = ps;
    a.scale = ps > 1 ? 2.0f / (float)(ps - 1) : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    if (ps <= LDS_PS) {
        const int lds = (ps * (ps | 1) + 3 * ps) * (int)sizeof(float);
        CAE_TRY(ensure_lds((const void *)elastic_lds_kernel, lds));
        hipLaunchKernelGGL(elastic_lds_kernel, dim3((unsigned)(n * c)), dim3(256), (size_t)lds, st, a);
    } else {
        const int lds = rows * (ps | 1) * (int)sizeof(float);
        CAE_TRY(ensure_lds((const void *)prefilter_rows_kernel, lds));
        hipLaunchKernelGGL(prefilter_rows_kernel, dim3((unsigned)((long)n * c * row_strips)), dim3(256), (size_t)lds, st, x_in,
                           a.ws, ps, rows, (int)row_strips);
        const int lds_cols = ps * cols * (int)sizeof(float);
        CAE_TRY(ensure_lds((const void *)prefilter_columns_kernel, lds_cols));
        hipLaunchKernelGGL(prefilter_columns_kernel, dim3((unsigned)((long)n * c * col_strips)), dim3(256), (size_t)lds_cols, st,
                           a.ws, ps, cols, (int)col_strips);
        switch (c) {
            case 1: launch_global<1>(a, n, (int)strips, st); break;
            case 2: launch_global<2>(a, n, (int)strips, st); break;
            case 3: launch_global<3>(a, n, (int)strips, st); break;
            default: launch_global<4>(a, n, (int)strips, st); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
