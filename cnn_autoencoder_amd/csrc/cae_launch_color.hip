// Launchers of the small colour-layer kernel (cae_kernels_color.hpp) and of the uint8 conversion behind the generic
// colour launch; see cae_launch.hpp
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"
#include "cae_kernels_color.hpp"
namespace cae {

template <int KS, bool SPLIT>
static int launch_color_small_t(const ColorArgs &a, hipStream_t st) {
    const unsigned grid = (unsigned)((size_t)a.N * a.tiles_x * a.tiles_y);
    hipLaunchKernelGGL((color_small_kernel<KS, SPLIT>), dim3(grid), dim3(COLOR_NW * 64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_color_small(int ks, bool split, const void *in, int in_planes, int cin, const float *w, const float *bias,
                       int n, int h, int w_px, int cout, void *out, int outfmt, int *flag, hipStream_t st) {
    if (cin < 1 || cin > 128 || cout < 1 || cout > 4)
        return fail(CAE_ERR_UNSUPPORTED, "small colour kernel: %d -> %d channels not covered", cin, cout);
    ColorArgs a{};
    a.in = in;
    a.out = out;
    a.w = w;
    a.bias = bias;
    a.N = n;
    a.H = h;
    a.W = w_px;
    a.in_planes = in_planes;
    a.chunks = (cin + 7) / 8;
    a.cout = cout;
    a.tiles_x = (w_px + COLOR_TX - 1) / COLOR_TX;
    a.tiles_y = (h + COLOR_TY - 1) / COLOR_TY;
    a.outfmt = outfmt;
    a.flag = flag;
    if ((size_t)n * a.tiles_x * a.tiles_y > 0x7fffffffu) return fail(CAE_ERR_ARG, "colour layer grid too large");
    if (ks == 3) return split ? launch_color_small_t<3, true>(a, st) : launch_color_small_t<3, false>(a, st);
    if (ks == 5) return split ? launch_color_small_t<5, true>(a, st) : launch_color_small_t<5, false>(a, st);
    return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks);
}

int launch_nchw_to_u8hwc(const float *in, void *out, int n, int c, size_t hw, hipStream_t st) {
    const size_t total = (size_t)n * hw * c;
    const size_t blocks = std::min<size_t>(std::max<size_t>((total + 255) / 256, 1), 256 * 8 * 4);
    hipLaunchKernelGGL(nchw_to_u8hwc_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in, (uint8_t *)out, n, c, hw);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // namespace cae
