// Launchers of the segmentation head's kernels (cae_launch_seg.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace cae {
struct SegConvArgs;
// seg_conv_f16_kernel<ks, ct> over `groups` groups of ct channel tiles; fills tiles_x / tiles_y from the kernel's tile
int launch_seg_conv(int ks, int ct, int groups, const SegConvArgs &a, hipStream_t st);
int launch_seg_finalize(const float *stats, int tiles, int n, int cp, const float *gamma, const float *beta, float *ab,
                        hipStream_t st);
int launch_seg_plane_moments(const float *x, int n, int c, int cp, size_t hw, const float *gamma, const float *beta,
                             float *ab, hipStream_t st);
int launch_seg_nchw_to_c8(const float *in, float *out, int n, int c, size_t hw, hipStream_t st);
int launch_seg_c8_to_nchw(const float *in, float *out, int n, int c, size_t hw, hipStream_t st);
// cae_seg_train.hip: pack_seg_f16 on the device (w a device fp32 weight, out device halves), and the padded vectors of a
// layer (bias rows, gamma, beta); a value outside the f16 range raises *flag (pad_vec: when `guard`)
int launch_seg_pack_dev(const float *w, int cin_a, int cin_b, int cout, int ks, bool up, void *out, int *flag,
                        hipStream_t st);
int launch_seg_pad_vec(const float *src, int c, bool up, int total, bool guard, float *dst, int *flag, hipStream_t st);
}  // namespace cae
