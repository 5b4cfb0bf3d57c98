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
}  // namespace cae
