// Differentiable MS-SSIM for the training objective (DistMSSSIMLoss of the reference, _ratedist.py:66-90, which calls
// pytorch_msssim.ms_ssim): one scale of the index forward, its adjoint with respect to the reconstruction, and the
// adjoint of the 2 x 2 average pooling between scales.
//
// Planar fp32 images, `planes` = N * C images of h x w.  X is the reconstruction (it carries the gradient), Y the target.
// Forward: msssim_level_kernel (cae_kernels.hpp) generalised to the window sizes 1..11 and to C1 / C2 arguments, with the
// moments in float64: the Gaussian is applied separably without padding, rows first; per 32 x 32 tile of the
// (h-win+1) x (w-win+1) maps one float64 partial of the ssim map and of the contrast-structure (cs) map, summed in a fixed order by msssim_sum_kernel.
// Backward, two launches with three coefficient maps in HBM between them:
//   1. msssim_tile_kernel<WIN, true> recomputes the local moments (mu_x, mu_y, E[x^2], E[y^2], E[xy]) and writes
//      A = dJ/dmu_x, B = dJ/dE[x^2], Cc = dJ/dE[xy] per map pixel, J = (g_ssim * sum ssim + g_cs * sum cs) / pixels;
//   2. msssim_gather_kernel<WIN> applies the transpose of the valid separable filter (a full correlation) to the three
//      maps and accumulates G_X += Gt(A) + 2 X Gt(B) + Y Gt(Cc).
// Every output pixel is owned by one thread and no atomics are used: forward and backward are bitwise reproducible.
// Both passes are register-blocked: a thread forms 4 neighbouring outputs from one run of win + 3 LDS reads.
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"

#include <hip/hip_runtime.h>

using namespace cae;

namespace {

constexpr int T = 32;       // outputs per tile side
constexpr int RB = 4;       // outputs per thread and pass
constexpr int MAX_WIN = 11;

struct Taps {
    double g[MAX_WIN];  // float64 taps: the moments are formed in float64 (see msssim_tile_kernel)
    float f[MAX_WIN];   // the same taps rounded, for the gather of the float32 coefficient maps
};

// One block = one 32 x 32 tile of the maps of one plane.  The images are float32; the five local moments and the two index
// maps are formed in float64: ssim's variances E[x^2] - mu^2 cancel to a small fraction of their terms (to ~1e-3 of them
// under the narrow windows of the coarse pyramid levels), and float32 moments left the means of small maps a few 1e-5 from
// float64.  Products of two floats are exact in float64, so what is left is the rounding of the float64 sums.
//   COEF = false: part[(plane * bpp + blk) * 2 + {0: ssim, 1: cs}] = float64 sums over the tile
//   COEF = true:  maps[(q * planes + plane) * OH * OW + pixel], q = 0: A, 1: B, 2: Cc
template <int WIN, bool COEF>
__global__ void __launch_bounds__(256)
msssim_tile_kernel(const float *X, const float *Y, int planes, int H, int W, int bx_per_row, int bpp, const Taps taps,
                   double C1, double C2, const double *g_ssim, const double *g_cs, double *part, float *maps) {
    // Pitch IN + 1 as in the metric kernel.  NOT conflict-free here: measured at win 11 (16 x 3 x 256^2), bank-conflict cycles
    // are 0.38 (forward) and 0.40 (coefficients) of the LDS-active cycles of this kernel and 0.26 of the gather's
    // (profiles/msssim_train/lds_bank_conflicts.txt).  Which access causes them has not been located.
    constexpr int IN = T + WIN - 1, P = IN + 1;
    __shared__ float sx[IN][P], sy[IN][P];
    __shared__ double vs[5][T][P];  // after the vertical pass: [quantity][out row][in col]; later the staged A, B, Cc (float)
    __shared__ double red[COEF ? 1 : 2][COEF ? 1 : 256];
    const int tid = threadIdx.x;
    const int plane = blockIdx.y, blk = blockIdx.x;
    const int by = blk / bx_per_row, bx = blk - by * bx_per_row;
    const int oy0 = by * T, ox0 = bx * T;
    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const float *px = X + (size_t)plane * H * W, *py = Y + (size_t)plane * H * W;
    for (int i = tid; i < IN * IN; i += 256) {
        const int r = i / IN, x = i - r * IN;
        const int iy = oy0 + r, ix = ox0 + x;
        const bool ok = iy < H && ix < W;
        sx[r][x] = ok ? px[(size_t)iy * W + ix] : 0.f;
        sy[r][x] = ok ? py[(size_t)iy * W + ix] : 0.f;
    }
    __syncthreads();
    // dimension 2 (rows) first, as pytorch_msssim's gaussian_filter does; 4 output rows per thread
    for (int i = tid; i < (T / RB) * IN; i += 256) {
        const int yb = i / IN, x = i - yb * IN;
        double acc[5][RB];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < RB; ++j) acc[q][j] = 0.0;
#pragma unroll
        for (int r = 0; r < WIN + RB - 1; ++r) {
            const double u = (double)sx[yb * RB + r][x], v = (double)sy[yb * RB + r][x];
            const double uu = u * u, vv = v * v, uv = u * v;  // exact
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int k = r - j;
                if (k >= 0 && k < WIN) {
                    const double w = taps.g[k];
                    acc[0][j] += w * u;
                    acc[1][j] += w * v;
                    acc[2][j] += w * uu;
                    acc[3][j] += w * vv;
                    acc[4][j] += w * uv;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int j = 0; j < RB; ++j) vs[q][yb * RB + j][x] = acc[q][j];
    }
    __syncthreads();
    // columns: thread -> row y, outputs x0 .. x0 + 3
    const int y = tid >> 3, x0 = (tid & 7) * RB;
    double m[5][RB];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
#pragma unroll
        for (int j = 0; j < RB; ++j) m[q][j] = 0.0;
#pragma unroll
        for (int r = 0; r < WIN + RB - 1; ++r) {
            const double v = vs[q][y][x0 + r];
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int k = r - j;
                if (k >= 0 && k < WIN) m[q][j] += taps.g[k] * v;
            }
        }
    }
    double gs = 0.0, gc = 0.0;
    if constexpr (COEF) {
        const double pixels = (double)OH * OW;
        gs = g_ssim ? g_ssim[plane] / pixels : 0.0;
        gc = g_cs ? g_cs[plane] / pixels : 0.0;
        __syncthreads();  // every thread has read its run of vs: reuse it as the staging tile
    }
    double ssum = 0.0, csum = 0.0;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const bool ok = oy0 + y < OH && ox0 + x0 + j < OW;
        const double mu1 = m[0][j], mu2 = m[1][j];
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const double s1 = m[2][j] - mu1_sq, s2 = m[3][j] - mu2_sq, s12 = m[4][j] - mu12;
        const double dc = s1 + s2 + C2, dl = mu1_sq + mu2_sq + C1;
        const double cs = (2.0 * s12 + C2) / dc;
        const double lum = (2.0 * mu12 + C1) / dl;
        if constexpr (!COEF) {
            if (ok) {
                ssum += lum * cs;
                csum += cs;
            }
        } else {
            // J = gs * lum * cs + gc * cs per pixel; k = dJ/dcs
            const double k = gs * lum + gc;
            const double rdc = 1.0 / dc, rdl = 1.0 / dl;
            float *st = reinterpret_cast<float *>(&vs[0][0][0]);
            st[(0 * T + y) * T + x0 + j] = (float)(gs * cs * 2.0 * rdl * (mu2 - lum * mu1) + k * 2.0 * rdc * (cs * mu1 - mu2));
            st[(1 * T + y) * T + x0 + j] = (float)(-k * cs * rdc);
            st[(2 * T + y) * T + x0 + j] = (float)(2.0 * k * rdc);
        }
    }
    if constexpr (!COEF) {
        red[0][tid] = ssum;
        red[1][tid] = csum;
        __syncthreads();
#pragma unroll
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                red[0][tid] += red[0][tid + s];
                red[1][tid] += red[1][tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            part[((size_t)plane * bpp + blk) * 2 + 0] = red[0][0];
            part[((size_t)plane * bpp + blk) * 2 + 1] = red[1][0];
        }
    } else {
        __syncthreads();
        const float *st = reinterpret_cast<const float *>(&vs[0][0][0]);
        const size_t map = (size_t)OH * OW;
        for (int i = tid; i < 3 * T * T; i += 256) {  // one 128-byte row segment per 32 lanes
            const int q = i / (T * T), r = (i / T) % T, c = i % T;
            if (oy0 + r < OH && ox0 + c < OW)
                maps[((size_t)q * planes + plane) * map + (size_t)(oy0 + r) * OW + ox0 + c] = st[i];
        }
    }
}

// out[plane * 2 + j] = sum of the block partials (fixed order) / samples
__global__ void __launch_bounds__(256) msssim_sum_kernel(const double *part, int bpp, double samples, double *out) {
    __shared__ double red[2][256];
    const int plane = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = tid; i < bpp; i += 256) {
        a += part[((size_t)plane * bpp + i) * 2 + 0];
        b += part[((size_t)plane * bpp + i) * 2 + 1];
    }
    red[0][tid] = a;
    red[1][tid] = b;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[(size_t)plane * 2 + 0] = red[0][0] / samples;
        out[(size_t)plane * 2 + 1] = red[1][0] / samples;
    }
}

// One block = 32 x 32 pixels of G_X of one plane: Gt(M)[i][j] = sum_ab g[a] g[b] M[i - a][j - b], M zero outside the map.
template <int WIN>
__global__ void __launch_bounds__(256)
msssim_gather_kernel(const float *X, const float *Y, const float *maps, int planes, int H, int W, int bx_per_row,
                     const Taps taps, float *GX) {
    constexpr int IN = T + WIN - 1, P = IN + 1;
    __shared__ float sm[3][IN][P];  // the maps from (oy0 - WIN + 1, ox0 - WIN + 1); later the staged Gt(A), Gt(B), Gt(Cc)
    __shared__ float vs[3][T][P];
    const int tid = threadIdx.x;
    const int plane = blockIdx.y, blk = blockIdx.x;
    const int by = blk / bx_per_row, bx = blk - by * bx_per_row;
    const int oy0 = by * T, ox0 = bx * T;
    const int OH = H - WIN + 1, OW = W - WIN + 1;
    const size_t map = (size_t)OH * OW;
    for (int i = tid; i < 3 * IN * IN; i += 256) {
        const int q = i / (IN * IN), r = (i / IN) % IN, c = i % IN;
        const int my = oy0 - (WIN - 1) + r, mx = ox0 - (WIN - 1) + c;
        const bool ok = my >= 0 && my < OH && mx >= 0 && mx < OW;
        sm[q][r][c] = ok ? maps[((size_t)q * planes + plane) * map + (size_t)my * OW + mx] : 0.f;
    }
    __syncthreads();
    // out[y] = sum_a g[a] M[y - a] = sum_k g[WIN - 1 - k] sm[y + k]
    for (int i = tid; i < 3 * (T / RB) * IN; i += 256) {
        const int q = i / ((T / RB) * IN), yb = (i / IN) % (T / RB), x = i % IN;
        float acc[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) acc[j] = 0.f;
#pragma unroll
        for (int r = 0; r < WIN + RB - 1; ++r) {
            const float v = sm[q][yb * RB + r][x];
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int k = r - j;
                if (k >= 0 && k < WIN) acc[j] += taps.f[WIN - 1 - k] * v;
            }
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) vs[q][yb * RB + j][x] = acc[j];
    }
    __syncthreads();
    const int y = tid >> 3, x0 = (tid & 7) * RB;
    float *st = &sm[0][0][0];  // 3 * T * T <= 3 * IN * P; sm was last read before the barrier above
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float m[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) m[j] = 0.f;
#pragma unroll
        for (int r = 0; r < WIN + RB - 1; ++r) {
            const float v = vs[q][y][x0 + r];
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int k = r - j;
                if (k >= 0 && k < WIN) m[j] += taps.f[WIN - 1 - k] * v;
            }
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) st[(q * T + y) * T + x0 + j] = m[j];
    }
    __syncthreads();
    const size_t base = (size_t)plane * H * W;
    for (int i = tid; i < T * T; i += 256) {
        const int r = i / T, c = i - r * T;
        const int iy = oy0 + r, ix = ox0 + c;
        if (iy < H && ix < W) {
            const size_t o = base + (size_t)iy * W + ix;
            GX[o] += st[i] + 2.f * X[o] * st[T * T + i] + Y[o] * st[2 * T * T + i];
        }
    }
}

// fine[y][x] = coarse[(y + ph) / 2][(x + pw) / 2] / 4: the adjoint of avgpool2_kernel (padded samples counted)
__global__ void __launch_bounds__(256)
avgpool2_bwd_kernel(const float *coarse, float *fine, int planes, int H, int W, int OH, int OW) {
    const int ph = H & 1, pw = W & 1;
    const size_t total = (size_t)planes * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const size_t pl = i / ((size_t)W * H);
        fine[i] = 0.25f * coarse[(pl * OH + ((y + ph) >> 1)) * OW + ((x + pw) >> 1)];
    }
}

int check_level(const float *x, const float *y, int planes, int h, int w, const double *taps, int win) {
    if (!x || !y || !taps) return fail(CAE_ERR_ARG, "NULL argument");
    if (planes < 1 || planes > 65535) return fail(CAE_ERR_ARG, "%d planes: 1..65535 are built (one grid row per plane)", planes);
    if (win < 1 || win > MAX_WIN || !(win & 1)) return fail(CAE_ERR_ARG, "window size %d: odd sizes 1..11 are built", win);
    if (h < win || w < win) return fail(CAE_ERR_ARG, "image smaller than the %d-tap window", win);
    return CAE_OK;
}

int tiles(int n) { return (n + T - 1) / T; }

Taps make_taps(const double *taps_host, int win) {
    Taps t = {};
    for (int i = 0; i < win; ++i) {
        t.g[i] = taps_host[i];
        t.f[i] = (float)taps_host[i];
    }
    return t;
}

unsigned ew_blocks(size_t total) {
    const size_t b = (total + 255) / 256;
    return (unsigned)(b < 65536 ? b : 65536);
}

// expands to one launch per built window size
#define MSSSIM_DISPATCH(win, LAUNCH) \
    switch (win) {                   \
        case 1: LAUNCH(1); break;    \
        case 3: LAUNCH(3); break;    \
        case 5: LAUNCH(5); break;    \
        case 7: LAUNCH(7); break;    \
        case 9: LAUNCH(9); break;    \
        default: LAUNCH(11); break;  \
    }

}  // namespace

extern "C" {

int cae_t_msssim_level_fwd(const float *x, const float *y, int planes, int h, int w, const double *taps_host, int win,
                           double c1, double c2, double *ssim_cs, double *workspace, size_t workspace_elems, void *stream) {
    CAE_TRY(check_level(x, y, planes, h, w, taps_host, win));
    if (!ssim_cs || !workspace) return fail(CAE_ERR_ARG, "NULL argument");
    const int oh = h - win + 1, ow = w - win + 1;
    const int bxr = tiles(ow), bpp = bxr * tiles(oh);
    if (workspace_elems < (size_t)planes * bpp * 2)
        return fail(CAE_ERR_ARG, "workspace too small: %zu doubles needed", (size_t)planes * bpp * 2);
    const Taps t = make_taps(taps_host, win);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(WIN)                                                                                                  \
    hipLaunchKernelGGL((msssim_tile_kernel<WIN, false>), dim3(bpp, planes), dim3(256), 0, st, x, y, planes, h, w, bxr, \
                       bpp, t, c1, c2, (const double *)nullptr, (const double *)nullptr, workspace, (float *)nullptr)
    MSSSIM_DISPATCH(win, LAUNCH)
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(msssim_sum_kernel, dim3(planes), dim3(256), 0, st, workspace, bpp, (double)oh * ow, ssim_cs);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_t_msssim_level_bwd(const float *x, const float *y, int planes, int h, int w, const double *taps_host, int win,
                           double c1, double c2, const double *g_ssim, const double *g_cs, float *gx, float *workspace,
                           size_t workspace_elems, void *stream) {
    CAE_TRY(check_level(x, y, planes, h, w, taps_host, win));
    if (!gx || !workspace) return fail(CAE_ERR_ARG, "NULL argument");
    const int oh = h - win + 1, ow = w - win + 1;
    if (workspace_elems < (size_t)3 * planes * oh * ow)
        return fail(CAE_ERR_ARG, "workspace too small: %zu floats needed", (size_t)3 * planes * oh * ow);
    const Taps t = make_taps(taps_host, win);
    hipStream_t st = (hipStream_t)stream;
    const int bxr = tiles(ow), bpp = bxr * tiles(oh);
#define LAUNCH(WIN)                                                                                                 \
    hipLaunchKernelGGL((msssim_tile_kernel<WIN, true>), dim3(bpp, planes), dim3(256), 0, st, x, y, planes, h, w, bxr, \
                       bpp, t, c1, c2, g_ssim, g_cs, (double *)nullptr, workspace)
    MSSSIM_DISPATCH(win, LAUNCH)
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    const int gxr = tiles(w), gpp = gxr * tiles(h);
#define LAUNCH(WIN)                                                                                                  \
    hipLaunchKernelGGL((msssim_gather_kernel<WIN>), dim3(gpp, planes), dim3(256), 0, st, x, y, (const float *)workspace, \
                       planes, h, w, gxr, t, gx)
    MSSSIM_DISPATCH(win, LAUNCH)
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_t_avgpool2_bwd(const float *g_coarse, int planes, int h, int w, float *g_fine, void *stream) {
    if (!g_coarse || !g_fine) return fail(CAE_ERR_ARG, "NULL argument");
    if (planes < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad shape");
    const int oh = (h + 2 * (h & 1) - 2) / 2 + 1, ow = (w + 2 * (w & 1) - 2) / 2 + 1;
    hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3(ew_blocks((size_t)planes * h * w)), dim3(256), 0, (hipStream_t)stream,
                       g_coarse, g_fine, planes, h, w, oh, ow);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // extern "C"
