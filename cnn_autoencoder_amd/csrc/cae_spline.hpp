// What the spline resamplers share: the recursive inverse filter of a B-spline along one line and the half-sample
// symmetric reflection of an index (cae_sampler.hip: quartic rotation; cae_elastic.hip: cubic elastic deformation).
#pragma once
#include <hip/hip_runtime.h>

namespace cae {

// One pole over the line c[0], c[stride], ..., n values, in place; `gain` scales the line on the way in.  The start of the
// causal recursion sums z^i over the whole line: the caller drops the terms from START_TERMS on, and takes z^n for 0
// above POWER_TERMS, where they lie below float32 resolution for its pole.
template <int START_TERMS, int POWER_TERMS>
__device__ __forceinline__ void filter_pole(float *c, int n, int stride, float z, float gain) {
    float zn = 1.0f;
    for (int i = 0; i < min(n, POWER_TERMS); ++i) zn *= z;
    if (n > POWER_TERMS) zn = 0.0f;
    const float c0 = gain * c[0];
    float acc = c0 + zn * (gain * c[(n - 1) * stride]), zi = z;
    const int terms = min(n, START_TERMS);
    for (int i = 1; i < terms; ++i) {
        acc += zi * (gain * (c[i * stride] + zn * c[(n - 1 - i) * stride]));
        zi *= z;
    }
    float v = c0 + z / (1.0f - zn * zn) * acc;
    c[0] = v;
    for (int i = 1; i < n; ++i) {
        v = gain * c[i * stride] + z * v;
        c[i * stride] = v;
    }
    v *= z / (z - 1.0f);
    c[(n - 1) * stride] = v;
    for (int i = n - 2; i >= 0; --i) {
        v = z * (v - c[i * stride]);
        c[i * stride] = v;
    }
}

// d c b a | a b c d | d c b a, as often as needed (the callers clamp coordinates, so |idx| is at most a few n)
__device__ __forceinline__ int reflect(int idx, int n) {
    int m = idx % (2 * n);
    if (m < 0) m += 2 * n;
    return m >= n ? 2 * n - 1 - m : m;
}

}  // namespace cae
