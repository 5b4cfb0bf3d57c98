// Launchers of the kernel families; each is defined in its own translation unit (cae_launch_*.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <utility>

#include "cae_hip.h"
#include "cae_internal.hpp"

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return ::cae::fail(CAE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// returns a CAE_* error code early
#define CAE_TRY(expr)                          \
    do {                                       \
        const int rc_ = (expr);                \
        if (rc_ != CAE_OK) return rc_;         \
    } while (0)

namespace cae {
// Guards the per-device launch state below (and the training path's zero pages).
inline std::mutex &launch_mutex() {
    static std::mutex mu;
    return mu;
}

// Raises `kernel`'s dynamic LDS limit on the current device to at least `bytes` (the attribute is per device; it is set
// once per kernel, device and larger size).
inline int ensure_lds(const void *kernel, int bytes) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static std::map<std::pair<const void *, int>, int> seen;  // (kernel, device) -> bytes set
    std::lock_guard<std::mutex> lock(launch_mutex());
    int &have = seen[{kernel, dev}];
    if (have < bytes) {
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        have = bytes;
    }
    return CAE_OK;
}

// Compute units of the current device, into `cus` (sizes the persistent grids).
inline int device_cus(int &cus) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static std::map<int, int> known;
    std::lock_guard<std::mutex> lock(launch_mutex());
    auto it = known.find(dev);
    if (it == known.end()) {
        int n = 0;
        HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        it = known.emplace(dev, n).first;
    }
    cus = it->second;
    return CAE_OK;
}

// The launch facts of a kernel live with its launcher: the caller leaves tiles_x, tiles_y and cci of its LayerArgs
// alone, the launcher fills them into a copy from its kernel's tile (tx x ty pixels of the w x h extent the grid
// covers) and contraction chunk (`cci` chunks of the `cin` real input channels the caller names).
template <class Args>
Args with_launch_facts(const Args &a, int w, int h, int tx, int ty, int cci) {
    Args b = a;
    b.tiles_x = (w + tx - 1) / tx;
    b.tiles_y = (h + ty - 1) / ty;
    b.cci = cci;
    return b;
}

struct LayerArgs;
struct FirstArgs;
int launch_conv(int ks, int ct, bool gdn, int cin, const LayerArgs &a, hipStream_t st);
int launch_conv_s1(int ks, int ct, bool zeropad, bool gdn, int cin, const LayerArgs &a, hipStream_t st);
int launch_deconv(int ks, int ct, bool gdn, int cin, const LayerArgs &a, hipStream_t st);
int launch_gdn(int ct, bool inverse, const LayerArgs &a, hipStream_t st);
int launch_first(int ks, int ct, bool gdn, const LayerArgs &a, const FirstArgs &f, hipStream_t st);
int launch_last(int ks, int cin, const LayerArgs &a, hipStream_t st);
int launch_conv_f16(int ks, int ct, bool gdn, int cin, const LayerArgs &a, hipStream_t st);
int launch_deconv_f16(int ks, int ct, bool gdn, int cin, const LayerArgs &a, hipStream_t st);
int launch_conv_s1_f16(int ks, int ct, bool synthesis, bool gdn, int cin, const LayerArgs &a, hipStream_t st);
int launch_color_f16(int ks, int cin, const LayerArgs &a, hipStream_t st);
// Do the split-f16 kernels of an analysis layer (conv_s2_f16_kernel<ks, ct, gdn>) / of the last synthesis layer
// (deconv_last_f16_kernel, all `cin` channels' weights resident) fit the LDS?  A layer that does not runs on the fp32 /
// the generic transposed-convolution kernel instead.
bool conv_f16_fits(int ks, int ct, bool gdn);
bool last_f16_fits(int ks, int cin);
// colour layer from <= 128 channels (C8 rows, or C8SP rows when `split`) to <= 4 image channels, fp32 NCHW / uint8 HWC out
int launch_color_small(int ks, bool split, const void *in, int in_planes, int cin, const float *w, const float *bias,
                       int n, int h, int w_px, int cout, void *out, int outfmt, int *flag, hipStream_t st);
// fp32 NCHW -> uint8 HWC with the x255 / clip / truncate epilogue
int launch_nchw_to_u8hwc(const float *in, void *out, int n, int c, size_t hw, hipStream_t st);
int launch_first_f16(int ks, int ct, bool gdn, const LayerArgs &a, const FirstArgs &f, hipStream_t st);
int launch_last_f16(int ks, int cin, const LayerArgs &a, hipStream_t st);
// GDN / IGDN in place on the split rows a.out (layers wider than 128 channels; a.outfmt must be OUT_C8)
int launch_gdn_f16(int ct, bool inverse, const LayerArgs &a, hipStream_t st);
}  // namespace cae
