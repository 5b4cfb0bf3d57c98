// Training input on the device: crop, noise, normalise and rotate patches out of a pool of uint8 HWC tiles in HBM,
// written as the fp32 NCHW batch train_step and the losses take (contract: include/cae_hip.h, cae_t_sample_patches).
//
// Reference: the per-patch CPU transform of utils/datasets/_augs.py:197-264 (get_zarr_transform, label_density == 0):
// ToTensor, AddGaussianNoise(0, 0.001), RandomCrop(pad_if_needed), Normalize(0.5, 0.5), bilinear RandomRotation.  The
// random draws (tile, offsets, angle) stay on the host (sampler.py); the kernels do the per-pixel work.
//
// Both kernels are output-stationary and exchange nothing between lanes: no LDS, no atomics.  The noise of a patch pixel
// is a pure function of (seed, sample index, patch pixel) -- Philox4x32-10, one evaluation gives the normals of all (at most
// four) channels -- so whichever output pixel reads a patch pixel sees the same value, and the result does not depend on
// the launch shape.
//   sample_rows_kernel<C, VEC>   no rotation: a thread takes 4 adjacent pixels of a patch row; inside the image that is
//                                one contiguous 4 C-byte read, and one 16-byte store per channel plane (VEC: ps % 4 == 0
//                                and a 16-byte aligned output; else dword stores with a tail)
//   sample_rotate_kernel<C>      rotation: one output pixel per thread, the four bilinear taps regenerated
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>

using namespace cae;

namespace {

struct SampleArgs {
    const uint8_t *pool;     // [T][H][W][C]
    const int32_t *tile_hw;  // [T][2] valid rows, columns of each tile, or null (H, W)
    const int32_t *tile, *y0, *x0;
    const float *cosa, *sina;  // null: no rotation
    float *out;                // [n][C][ps][ps]
    int T, H, W, ps;
    uint32_t key0, key1, sample_base;
    float noise_std;
    int normalize;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// -2 ln u for u = (w + 0.5) 2^-32.  In the upper half u = 1 - t with t = (~w + 0.5) 2^-32 exact enough in float32 where
// u itself is not (u rounds to 1 for w >= 2^32 - 128): log1pf keeps the radius of small normals to a few ulp.
__device__ __forceinline__ float neg2_log_u(uint32_t w) {
    const float u = ((float)w + 0.5f) * 0x1p-32f, t = ((float)~w + 0.5f) * 0x1p-32f;
    return -2.0f * ((w & 0x80000000u) ? log1pf(-t) : logf(u));
}

// normals 0, 1 from words 0, 1 and normals 2, 3 from words 2, 3 (Box-Muller: r cos 2 pi u', r sin 2 pi u')
template <int C>
__device__ __forceinline__ void normals(const SampleArgs &a, uint32_t sample, uint32_t pixel, float (&g)[4]) {
    uint32_t r[4];
    philox4x32_10(sample, pixel, 0u, 0u, a.key0, a.key1, r);
    float s, c;
    const float rad0 = sqrtf(neg2_log_u(r[0]));
    sincospif(((float)r[1] + 0.5f) * 0x1p-31f, &s, &c);
    g[0] = rad0 * c;
    g[1] = rad0 * s;
    if (C > 2) {
        const float rad1 = sqrtf(neg2_log_u(r[2]));
        sincospif(((float)r[3] + 0.5f) * 0x1p-31f, &s, &c);
        g[2] = rad1 * c;
        g[3] = rad1 * s;
    } else {
        g[2] = g[3] = 0.0f;
    }
}

// The placement of one sample: its offsets and its tile's valid extent.  Every value is clamped so that no index the
// kernels form can leave the pool or overflow, whatever the device arrays hold: a tile outside [0, T) has no valid pixel.
struct Placement {
    int y0, x0, hv, wv;
};

__device__ __forceinline__ Placement placement(const SampleArgs &a, int s) {
    Placement p;
    const int t = a.tile[s];
    const bool ok = t >= 0 && t < a.T;
    p.hv = ok ? a.H : 0;
    p.wv = ok ? a.W : 0;
    if (ok && a.tile_hw) {
        p.hv = min(max(a.tile_hw[2 * t], 0), a.H);
        p.wv = min(max(a.tile_hw[2 * t + 1], 0), a.W);
    }
    // offsets beyond (-ps, extent) select nothing but padding: clamping them keeps y0 + py inside int
    p.y0 = min(max(a.y0[s], -a.ps), a.H);
    p.x0 = min(max(a.x0[s], -a.ps), a.W);
    return p;
}

template <int C>
__device__ __forceinline__ const uint8_t *tile_base(const SampleArgs &a, int s) {
    const int t = a.tile[s];
    return a.pool + (size_t)((t >= 0 && t < a.T) ? t : 0) * a.H * a.W * C;
}

// v -> p of the contract: u8 / 255 correctly rounded (IEEE division), + noise, clamp, normalise
__device__ __forceinline__ float finish(const SampleArgs &a, uint8_t u8, float g) {
    float v = __fdiv_rn((float)u8, 255.0f);
    if (a.noise_std != 0.0f) v = fminf(fmaxf(v + a.noise_std * g, 0.0f), 1.0f);
    return a.normalize ? (v - 0.5f) / 0.5f : v;
}

// the C values p of patch pixel (py, px), 0 <= py, px < ps
template <int C>
__device__ __forceinline__ void patch_pixel(const SampleArgs &a, const Placement &pl, const uint8_t *img, uint32_t sample,
                                            int py, int px, float (&p)[C]) {
    const int iy = pl.y0 + py, ix = pl.x0 + px;
    if (iy >= 0 && iy < pl.hv && ix >= 0 && ix < pl.wv) {
        float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (a.noise_std != 0.0f) normals<C>(a, sample, (uint32_t)(py * a.ps + px), g);
        const uint8_t *src = img + ((size_t)iy * a.W + ix) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) p[ch] = finish(a, src[ch], g[ch]);
    } else {
        const float pad = a.normalize ? -1.0f : 0.0f;  // pad_if_needed's zeros, then Normalize
#pragma unroll
        for (int ch = 0; ch < C; ++ch) p[ch] = pad;
    }
}

template <int C, bool VEC>
__global__ void __launch_bounds__(256) sample_rows_kernel(const SampleArgs a, int strips) {
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int groups = (a.ps + 3) >> 2;
    const int item = strip * 256 + threadIdx.x;
    if (item >= a.ps * groups) return;
    const int py = item / groups, px = (item - py * groups) * 4;
    const Placement pl = placement(a, s);
    const uint8_t *img = tile_base<C>(a, s);
    const uint32_t sample = a.sample_base + (uint32_t)s;
    float p[4][C];
    const int iy = pl.y0 + py, ix = pl.x0 + px;
    if (iy >= 0 && iy < pl.hv && ix >= 0 && ix + 3 < pl.wv && px + 3 < a.ps) {
        uint8_t raw[4 * C];
        __builtin_memcpy(raw, img + ((size_t)iy * a.W + ix) * C, 4 * C);  // one contiguous read, any alignment
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.noise_std != 0.0f) normals<C>(a, sample, (uint32_t)(py * a.ps + px + k), g);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) p[k][ch] = finish(a, raw[k * C + ch], g[ch]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (px + k < a.ps) patch_pixel<C>(a, pl, img, sample, py, px + k, p[k]);
    }
    float *o = a.out + ((size_t)s * C * a.ps + py) * a.ps + px;
    const size_t plane = (size_t)a.ps * a.ps;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        if (VEC) {
            *reinterpret_cast<float4 *>(o + ch * plane) = make_float4(p[0][ch], p[1][ch], p[2][ch], p[3][ch]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (px + k < a.ps) o[ch * plane + k] = p[k][ch];
        }
    }
}

template <int C>
__global__ void __launch_bounds__(256) sample_rotate_kernel(const SampleArgs a, int strips) {
    const int s = blockIdx.x / strips, strip = blockIdx.x - s * strips;
    const int item = strip * 256 + threadIdx.x;
    if (item >= a.ps * a.ps) return;
    const int i = item / a.ps, j = item - i * a.ps;
    const Placement pl = placement(a, s);
    const uint8_t *img = tile_base<C>(a, s);
    const uint32_t sample = a.sample_base + (uint32_t)s;
    const float ca = a.cosa[s], sa = a.sina[s];
    const float c = 0.5f * (float)(a.ps - 1), dx = (float)j - c, dy = (float)i - c;
    const float sx = c + (ca * dx - sa * dy), sy = c + (sa * dx + ca * dy);
    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0f;
    // a source point outside (-1, ps) has no tap inside the patch (this also keeps NaN / huge coordinates out of the casts)
    if (sx > -1.0f && sx < (float)a.ps && sy > -1.0f && sy < (float)a.ps) {
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const int tx0 = (int)fx0, ty0 = (int)fy0;
        const float wx1 = sx - fx0, wy1 = sy - fy0, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ty = ty0 + (t >> 1), tx = tx0 + (t & 1);
            if (ty < 0 || ty >= a.ps || tx < 0 || tx >= a.ps) continue;  // zero fill
            const float w = ((t >> 1) ? wy1 : wy0) * ((t & 1) ? wx1 : wx0);
            float p[C];
            patch_pixel<C>(a, pl, img, sample, ty, tx, p);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] += w * p[ch];
        }
    }
    float *o = a.out + (size_t)s * C * a.ps * a.ps + item;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[(size_t)ch * a.ps * a.ps] = acc[ch];
}

template <int C>
void launch(const SampleArgs &a, int n, bool vec, hipStream_t st) {
    if (a.cosa) {
        const int strips = (a.ps * a.ps + 255) / 256;
        hipLaunchKernelGGL(sample_rotate_kernel<C>, dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
    } else {
        const int strips = (a.ps * ((a.ps + 3) / 4) + 255) / 256;
        if (vec)
            hipLaunchKernelGGL((sample_rows_kernel<C, true>), dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
        else
            hipLaunchKernelGGL((sample_rows_kernel<C, false>), dim3((unsigned)(n * strips)), dim3(256), 0, st, a, strips);
    }
}

}  // namespace

extern "C" int cae_t_sample_patches(const uint8_t *pool_dev, int tiles, int h, int w, int c, const int32_t *tile_hw_dev,
                                    const int32_t *tile_dev, const int32_t *y0_dev, const int32_t *x0_dev,
                                    const int32_t *tile_host, const float *cos_dev, const float *sin_dev, uint64_t seed,
                                    uint32_t sample_base, float noise_std, int normalize, int n, int ps, float *out_dev,
                                    void *stream) {
    if (c < 1 || c > 4) return fail(CAE_ERR_ARG, "1 to 4 channels per pixel, got %d", c);
    if (ps < 1 || ps > 16384) return fail(CAE_ERR_ARG, "patch size %d outside 1 .. 16384", ps);
    if (n < 0) return fail(CAE_ERR_ARG, "n = %d", n);
    if (tiles < 1 || h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24))
        return fail(CAE_ERR_ARG, "pool of %d tiles of %d x %d", tiles, h, w);
    if (!pool_dev || !tile_dev || !y0_dev || !x0_dev || !out_dev) return fail(CAE_ERR_ARG, "NULL argument");
    if ((cos_dev == nullptr) != (sin_dev == nullptr)) return fail(CAE_ERR_ARG, "cos and sin come together");
    if (!(noise_std >= 0.0f) || !(noise_std < 1e30f)) return fail(CAE_ERR_ARG, "noise_std must be finite and >= 0");
    if (tile_host)
        for (int s = 0; s < n; ++s)
            if (tile_host[s] < 0 || tile_host[s] >= tiles)
                return fail(CAE_ERR_ARG, "sample %d names tile %d of %d", s, tile_host[s], tiles);
    if (n == 0) return CAE_OK;
    const long strips = cos_dev ? ((long)ps * ps + 255) / 256 : ((long)ps * ((ps + 3) / 4) + 255) / 256;
    if ((long)n * strips > 0x7fffffffL) return fail(CAE_ERR_ARG, "%d patches of %d^2 in one call: split the batch", n, ps);
    SampleArgs a{};
    a.pool = pool_dev;
    a.tile_hw = tile_hw_dev;
    a.tile = tile_dev, a.y0 = y0_dev, a.x0 = x0_dev;
    a.cosa = cos_dev, a.sina = sin_dev;
    a.out = out_dev;
    a.T = tiles, a.H = h, a.W = w, a.ps = ps;
    a.key0 = (uint32_t)seed, a.key1 = (uint32_t)(seed >> 32), a.sample_base = sample_base;
    a.noise_std = noise_std;
    a.normalize = normalize != 0;
    const bool vec = ps % 4 == 0 && ((uintptr_t)out_dev & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    switch (c) {
        case 1: launch<1>(a, n, vec, st); break;
        case 2: launch<2>(a, n, vec, st); break;
        case 3: launch<3>(a, n, vec, st); break;
        default: launch<4>(a, n, vec, st); break;
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
