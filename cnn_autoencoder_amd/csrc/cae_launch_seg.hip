// Launchers of the segmentation head's kernels (cae_kernels_seg.hpp).
#include <algorithm>

#include "cae_kernels_seg.hpp"
#include "cae_launch.hpp"
#include "cae_launch_seg.hpp"

namespace cae {

template <int KS, int CT>
static int launch_seg_instance(const SegConvArgs &a, int groups, hipStream_t st) {
    using G = SegGeom<KS, CT>;
    CAE_TRY(ensure_lds((const void *)seg_conv_f16_kernel<KS, CT>, G::LDS_BYTES));
    const long blocks = (long)a.tiles_x * a.tiles_y * a.N;
    if (blocks > 0x7fffffffL || groups > 65535) return fail(CAE_ERR_ARG, "segmentation layer: grid too large");
    hipLaunchKernelGGL((seg_conv_f16_kernel<KS, CT>), dim3((unsigned)blocks, groups), dim3(256), G::LDS_BYTES, st, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_seg_conv(int ks, int ct, int groups, const SegConvArgs &args, hipStream_t st) {
    SegConvArgs a = args;  // the launch facts live here: the kernel's tile
    a.tiles_x = (args.W + SEG_TX - 1) / SEG_TX;
    a.tiles_y = (args.H + SEG_TY - 1) / SEG_TY;
    if (ks == 3 && ct == 1) return launch_seg_instance<3, 1>(a, groups, st);
    if (ks == 3 && ct == 2) return launch_seg_instance<3, 2>(a, groups, st);
    if (ks == 1 && ct == 1) return launch_seg_instance<1, 1>(a, groups, st);
    if (ks == 1 && ct == 2) return launch_seg_instance<1, 2>(a, groups, st);
    if (ks == 1 && ct == 4) return launch_seg_instance<1, 4>(a, groups, st);
    return fail(CAE_ERR_UNSUPPORTED, "no seg_conv_f16_kernel<%d, %d>", ks, ct);
}

int launch_seg_finalize(const float *stats, int tiles, int n, int cp, const float *gamma, const float *beta, float *ab,
                        hipStream_t st) {
    hipLaunchKernelGGL(seg_stats_finalize_kernel, dim3((n * cp + 255) / 256), dim3(256), 0, st, stats, tiles, n, cp, gamma,
                       beta, ab);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_seg_plane_moments(const float *x, int n, int c, int cp, size_t hw, const float *gamma, const float *beta,
                             float *ab, hipStream_t st) {
    hipLaunchKernelGGL(seg_plane_moments_kernel, dim3(n * cp), dim3(256), 0, st, x, c, cp, hw, gamma, beta, ab);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

static unsigned seg_ew_grid(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, 65535 * 16); }

int launch_seg_nchw_to_c8(const float *in, float *out, int n, int c, size_t hw, hipStream_t st) {
    const int planes = (c + 7) / 8;
    hipLaunchKernelGGL(nchw_to_c8_kernel, dim3(seg_ew_grid((size_t)n * planes * hw)), dim3(256), 0, st, in, out, n, c,
                       (int)hw, planes, (const int32_t *)nullptr, (const float *)nullptr);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_seg_c8_to_nchw(const float *in, float *out, int n, int c, size_t hw, hipStream_t st) {
    hipLaunchKernelGGL(c8_to_nchw_kernel, dim3(seg_ew_grid((size_t)n * c * hw)), dim3(256), 0, st, in, out, n, c, (int)hw,
                       (c + 7) / 8);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // namespace cae
