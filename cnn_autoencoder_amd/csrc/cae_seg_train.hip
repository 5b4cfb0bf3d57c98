// Backward pass of the segmentation head, per operation (cae_seg_pack_dev, cae_seg_conv2d, cae_seg_wgrad,
// cae_seg_norm_relu_backward, cae_seg_channel_sums; include/cae_hip.h): argument checks and launches.
#include <algorithm>
#include <climits>

#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_kernels_seg_train.hpp"
#include "cae_launch.hpp"
#include "cae_launch_seg.hpp"
#include "cae_pack.hpp"

namespace cae {

static unsigned ew_grid(size_t total) { return (unsigned)std::min<size_t>(std::max<size_t>((total + 255) / 256, 1), 65535 * 16); }
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int launch_seg_pack_dev(const float *w, int cin_a, int cin_b, int cout, int ks, bool up, void *out, int *flag,
                        hipStream_t st) {
    const int m = seg_rows(cout, up), ct = seg_ct(m, ks), chunks = seg_chunks(cin_a, cin_b);
    const size_t records = (size_t)seg_groups(m, ks) * chunks * ks * ks * ct;
    hipLaunchKernelGGL(seg_pack_dev_kernel, dim3(ew_grid(records * 512)), dim3(256), 0, st, w, cin_a, cin_b, cout, ks,
                       (int)up, ct, chunks, m, records, (_Float16 *)out, flag);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_seg_pad_vec(const float *src, int c, bool up, int total, bool guard, float *dst, int *flag, hipStream_t st) {
    const int cp = (c + 7) / 8 * 8;
    hipLaunchKernelGGL(seg_pad_vec_kernel, dim3((total + 255) / 256), dim3(256), 0, st, src, c, cp, seg_rows(c, up), (int)up,
                       total, (int)guard, dst, flag);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// The split rule of the weight gradient.  A launch has tiles = ceil(cout / 32) ceil(cin / 32) blocks per segment; the
// pixels are cut into as many segments as bring the grid to kWgTargetBlocks blocks (two per compute unit of an MI355X),
// while a segment keeps at least kWgMinSteps steps (four per wave) so that the merge does not outweigh the contraction.
constexpr long kWgTargetBlocks = 512, kWgMinSteps = 16, kWgMaxSplits = 1024;

struct WgradShape {
    long steps = 0, tiles = 0, per_seg = 0;
    int splits = 0, xs = 0;
    size_t total = 0;  // elements of gw
};

static bool wgrad_shape(int n, int h, int w, int cin, int cout, int ks, WgradShape &s) {
    if (n < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || (ks != 1 && ks != 3)) return false;
    if ((long)h * w > INT_MAX) return false;
    s.xs = (w + SEG_WG_K - 1) / SEG_WG_K;
    s.steps = (long)n * h * s.xs;
    s.tiles = (long)((cout + 31) / 32) * ((cin + 31) / 32);
    long k = (kWgTargetBlocks + s.tiles - 1) / s.tiles;
    k = std::min(k, std::max(1L, s.steps / kWgMinSteps));
    k = std::min(k, kWgMaxSplits);
    s.per_seg = (s.steps + k - 1) / k;
    s.splits = (int)((s.steps + s.per_seg - 1) / s.per_seg);
    s.total = (size_t)cout * cin * ks * ks;
    return (cout + 31) / 32 <= 65535;
}

struct Conv2dShape {
    int m, ct, groups, chunks, planes;
    size_t x_bytes, w_bytes, b_bytes;
};

static bool conv2d_shape(int n, int cin, int cout, int h, int w, int ks, Conv2dShape &s) {
    if (n < 1 || cin < 1 || cout < 1 || h < 1 || w < 1 || (ks != 1 && ks != 3) || (long)h * w > INT_MAX) return false;
    s.m = seg_rows(cout, false), s.ct = seg_ct(s.m, ks), s.groups = seg_groups(s.m, ks), s.chunks = seg_chunks(cin, 0);
    s.planes = (cin + 7) / 8;
    s.x_bytes = align256((size_t)n * s.planes * h * w * 32);
    s.w_bytes = align256(cae_seg_packed_halves(cin, 0, cout, ks, 0) * 2);
    s.b_bytes = align256((size_t)s.groups * s.ct * 32 * 4);
    return true;
}

}  // namespace cae

using namespace cae;

extern "C" {

int cae_seg_pack_dev(const float *w_dev, int cin_a, int cin_b, int cout, int ks, int up, uint16_t *out_dev, size_t capacity,
                     int *flag_dev, void *stream) {
    const size_t n = cae_seg_packed_halves(cin_a, cin_b, cout, ks, up);
    if (!w_dev || !out_dev) return fail(CAE_ERR_ARG, "NULL argument");
    if (!n) return fail(CAE_ERR_ARG, "cae_seg_pack_dev: cin_a, cin_b >= 0 (sum >= 1), cout >= 1, ks 1 or 3; the transposed form has ks 1 and one source");
    if (capacity < n) return fail(CAE_ERR_ARG, "cae_seg_pack_dev: %zu halves needed, room for %zu", n, capacity);
    return launch_seg_pack_dev(w_dev, cin_a, cin_b, cout, ks, up != 0, out_dev, flag_dev, (hipStream_t)stream);
}

size_t cae_seg_conv2d_workspace(int n, int cin, int cout, int h, int w, int ks) {
    Conv2dShape s;
    if (!conv2d_shape(n, cin, cout, h, w, ks, s)) return 0;
    return s.x_bytes + s.w_bytes + s.b_bytes;
}

int cae_seg_conv2d(const float *x_dev, const float *ab_dev, const float *w_dev, const float *bias_dev, int n, int cin,
                   int cout, int h, int w, int ks, float *out_dev, int *flag_dev, void *workspace_dev,
                   size_t workspace_bytes, void *stream) {
    if (n == 0) return CAE_OK;
    Conv2dShape s;
    if (!conv2d_shape(n, cin, cout, h, w, ks, s))
        return fail(CAE_ERR_ARG, "cae_seg_conv2d: n, cin, cout, h, w >= 1 and ks 1 or 3 (got %d, %d, %d, %d, %d, %d)", n, cin, cout, h, w, ks);
    if (!x_dev || !w_dev || !out_dev || !flag_dev || !workspace_dev) return fail(CAE_ERR_ARG, "cae_seg_conv2d: NULL argument");
    if (workspace_bytes < s.x_bytes + s.w_bytes + s.b_bytes || ((uintptr_t)workspace_dev & 15))
        return fail(CAE_ERR_ARG, "cae_seg_conv2d: workspace of %zu bytes, 16-byte aligned, needed", s.x_bytes + s.w_bytes + s.b_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    float *xc8 = (float *)ws, *bias = (float *)(ws + s.x_bytes + s.w_bytes);
    char *wp = ws + s.x_bytes;
    CAE_TRY(launch_seg_nchw_to_c8(x_dev, xc8, n, cin, (size_t)h * w, st));
    CAE_TRY(launch_seg_pack_dev(w_dev, cin, 0, cout, ks, false, wp, flag_dev, st));
    if (bias_dev) CAE_TRY(launch_seg_pad_vec(bias_dev, cout, false, s.groups * s.ct * 32, false, bias, flag_dev, st));
    SegConvArgs a{};
    a.A = SegSrc{xc8, ab_dev, s.planes}, a.B = SegSrc{nullptr, nullptr, 0};
    a.wp = wp, a.bias = bias_dev ? bias : nullptr, a.out = out_dev, a.flag = flag_dev, a.stats = nullptr;
    a.N = n, a.H = h, a.W = w, a.chunks = s.chunks, a.cout = cout, a.out_planes = (cout + 7) / 8, a.outmode = SEG_OUT_NCHW;
    return launch_seg_conv(ks, s.ct, s.groups, a, st);
}

int cae_seg_wgrad_splits(int n, int h, int w, int cin, int cout, int ks) {
    WgradShape s;
    return wgrad_shape(n, h, w, cin, cout, ks, s) ? s.splits : 0;
}

size_t cae_seg_wgrad_workspace(int n, int h, int w, int cin, int cout, int ks) {
    WgradShape s;
    return wgrad_shape(n, h, w, cin, cout, ks, s) ? (size_t)s.splits * s.total * 4 : 0;
}

int cae_seg_wgrad(const float *g_dev, const float *xa_dev, const float *aba_dev, int cin_a, const float *xb_dev,
                  const float *abb_dev, int cin_b, int n, int cout, int h, int w, int ks, float *gw_dev, int *flag_dev,
                  void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (n == 0) return CAE_OK;
    WgradShape s;
    if (cin_a < 0 || cin_b < 0 || !wgrad_shape(n, h, w, cin_a + cin_b, cout, ks, s))
        return fail(CAE_ERR_ARG, "cae_seg_wgrad: n, h, w, cout >= 1, cin_a, cin_b >= 0 (sum >= 1), ks 1 or 3");
    if (!g_dev || !gw_dev || !flag_dev || !workspace_dev || (cin_a && !xa_dev) || (cin_b && !xb_dev))
        return fail(CAE_ERR_ARG, "cae_seg_wgrad: NULL argument");
    if (workspace_bytes < (size_t)s.splits * s.total * 4 || ((uintptr_t)workspace_dev & 3))
        return fail(CAE_ERR_ARG, "cae_seg_wgrad: workspace of %zu bytes needed", (size_t)s.splits * s.total * 4);
    hipStream_t st = (hipStream_t)stream;
    SegWgradArgs a{};
    a.g = g_dev;
    a.A = SegGradSrc{xa_dev, aba_dev, cin_a}, a.B = SegGradSrc{xb_dev, abb_dev, cin_b};
    a.part = (float *)workspace_dev, a.flag = flag_dev;
    a.N = n, a.H = h, a.W = w, a.cout = cout, a.xs = s.xs, a.steps = s.steps, a.per_seg = s.per_seg;
    a.vec = w % 4 == 0 && (((uintptr_t)g_dev | (uintptr_t)xa_dev | (uintptr_t)xb_dev) & 15) == 0;
    const dim3 grid((unsigned)((cin_a + cin_b + 31) / 32), (unsigned)((cout + 31) / 32), (unsigned)s.splits);
    if (ks == 3)
        hipLaunchKernelGGL(seg_wgrad_f16_kernel<3>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(seg_wgrad_f16_kernel<1>, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seg_wgrad_merge_kernel, dim3(ew_grid(s.total)), dim3(256), 0, st, (const float *)workspace_dev,
                       s.splits, s.total, gw_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

size_t cae_seg_norm_workspace(int n, int c) { return n < 1 || c < 1 ? 0 : (size_t)n * c * 32; }

int cae_seg_norm_relu_backward(const float *x_dev, const float *ab_dev, const float *gamma_dev, const float *gv_dev, int n,
                               int c, size_t hw, float *gx_dev, float *dgamma_dev, float *dbeta_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream) {
    if (n == 0) return CAE_OK;
    if (n < 1 || c < 1 || hw < 1 || hw > INT_MAX || (long)n * c > INT_MAX)
        return fail(CAE_ERR_ARG, "cae_seg_norm_relu_backward: n, c, hw >= 1, n c and hw < 2^31");
    if (!x_dev || !ab_dev || !gv_dev) return fail(CAE_ERR_ARG, "cae_seg_norm_relu_backward: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int cp = (c + 7) / 8 * 8;
    if (!gamma_dev) {
        if (!gx_dev) return fail(CAE_ERR_ARG, "cae_seg_norm_relu_backward: without gamma there is only g_x to compute");
        const size_t total = (size_t)n * c * hw;
        hipLaunchKernelGGL(seg_relu_backward_kernel, dim3(ew_grid(total)), dim3(256), 0, st, x_dev, ab_dev, gv_dev, c, cp, hw,
                           total, gx_dev);
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
    if (!dgamma_dev || !dbeta_dev || !workspace_dev) return fail(CAE_ERR_ARG, "cae_seg_norm_relu_backward: NULL argument");
    if (workspace_bytes < cae_seg_norm_workspace(n, c) || ((uintptr_t)workspace_dev & 7))
        return fail(CAE_ERR_ARG, "cae_seg_norm_relu_backward: workspace of %zu bytes, 8-byte aligned, needed", cae_seg_norm_workspace(n, c));
    double *stats = (double *)workspace_dev;
    hipLaunchKernelGGL(seg_norm_reduce_kernel, dim3(n * c), dim3(256), 0, st, x_dev, ab_dev, gv_dev, c, cp, hw, stats);
    HIP_TRY(hipGetLastError());
    const unsigned bx = gx_dev ? (unsigned)std::min<size_t>((hw + 1023) / 1024, 1024) : 1u;
    hipLaunchKernelGGL(seg_norm_apply_kernel, dim3(n * c, bx), dim3(256), 0, st, x_dev, ab_dev, gamma_dev, gv_dev,
                       (const double *)stats, n, c, cp, hw, gx_dev, dgamma_dev, dbeta_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

size_t cae_seg_channel_sums_workspace(int n, int c) { return n < 1 || c < 1 ? 0 : (size_t)n * c * 8; }

int cae_seg_channel_sums(const float *g_dev, int n, int c, size_t hw, float *out_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream) {
    if (n == 0) return CAE_OK;
    if (n < 1 || c < 1 || hw < 1 || (long)n * c > INT_MAX) return fail(CAE_ERR_ARG, "cae_seg_channel_sums: n, c, hw >= 1, n c < 2^31");
    if (!g_dev || !out_dev || !workspace_dev) return fail(CAE_ERR_ARG, "cae_seg_channel_sums: NULL argument");
    if (workspace_bytes < cae_seg_channel_sums_workspace(n, c) || ((uintptr_t)workspace_dev & 7))
        return fail(CAE_ERR_ARG, "cae_seg_channel_sums: workspace of %zu bytes, 8-byte aligned, needed", cae_seg_channel_sums_workspace(n, c));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_plane_sums_kernel, dim3(n * c), dim3(256), 0, st, g_dev, hw, (double *)workspace_dev);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seg_channel_sums_kernel, dim3((c + 255) / 256), dim3(256), 0, st, (const double *)workspace_dev, n, c, out_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // extern "C"
