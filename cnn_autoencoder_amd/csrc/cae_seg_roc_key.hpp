// The key and bin of a logit in the ROC histograms (include/cae_hip.h, "ROC histograms of a one-class head"): one text for
// cae_seg_roc_hist and cae_seg_object_roc_hist, so that the two histograms cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cae {

// order-preserving key of an fp32 logit, cut to its top `bits` bits (shift = 32 - bits).  -0 counts as +0 and NaN as key
// 0; in integers, so that no floating-point mode (denormals) has a say: x + 0.0f changes no other value
__device__ __forceinline__ uint32_t roc_bin(float x, int shift) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0;
    const uint32_t key = (u >> 31) ? ~u : (u | 0x80000000u);
    return (u & 0x7fffffffu) > 0x7f800000u ? 0u : key >> shift;
}

}  // namespace cae
