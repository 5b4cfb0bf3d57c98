// The bin of a score in the average-precision histograms (include/cae_hip.h, "Score histograms of a head of several
// classes"): one text for cae_seg_score_hist and whatever counts scores after it, so that histograms cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cae {

// order-preserving bin of an fp32 score in [0, 1], `bits` in 8..14, B = 2^bits bins: below 0.5 the top bits of s itself,
// from 0.5 on those of t = 1 - s counted down from B - 1, so that the resolution is relative at both ends.  NaN, -0 and
// everything <= 0 go to bin 0, everything >= 1 to bin B - 1.  In integers but for the one subtraction, which is exact
// (Sterbenz: 0.5 <= s <= 1), so that no floating-point mode (rounding, denormals) has a say.  bits_of(0.5f) = 0x3F000000
// < 2^30: either half stays inside B / 2 bins
__device__ __forceinline__ uint32_t score_bin(float s, int bits) {
    const uint32_t u = __float_as_uint(s);
    const int sh = 31 - bits;
    if ((u >> 31) || u > 0x7f800000u) return 0u;  // negatives, -0, NaN
    if (u < 0x3f000000u) return u >> sh;          // 0 <= s < 0.5
    const uint32_t B = 1u << bits;
    if (u >= 0x3f800000u) return B - 1;           // s >= 1 (+inf too) counts as 1: t = 0
    return B - 1 - (__float_as_uint(1.0f - s) >> sh);
}

}  // namespace cae
