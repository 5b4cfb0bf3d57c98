// Backward kernels of the segmentation head (JNet), per operation on the caller's NCHW fp32 tensors.
//
//   seg_wgrad_f16_kernel       weight gradient of a stride-1 zero-padded KS x KS convolution over up to two concatenated
//                              sources: gw[co][ci][ky][kx] = sum_{n,y,x} g[n,co,y,x] v[n,ci,y+ky-P,x+kx-P], f16x3 on
//                              v_mfma_f32_32x32x16_f16 with the contraction over pixels.  v is the forward's staged value,
//                              max(fmaf(a, x, b), 0) bit for bit as seg_conv_f16_kernel stages it (or x untransformed), zero
//                              outside the plane: padding pads v, not x.
//   seg_norm_reduce_kernel /   backward of v = relu(GN(x)) with one group per channel: the plane sums on a fixed tree with
//   seg_norm_apply_kernel      double accumulators, then the elementwise pass.
//   seg_channel_sums_kernel    per-channel sums of a gradient (bias gradients).
//   seg_pack_dev_kernel        device twin of pack_seg_f16 (cae_pack.cpp), byte for byte.
// No atomics, every merge in a fixed order: results are bitwise repeatable.
#pragma once
#include "cae_kernels_seg.hpp"

namespace cae {

// One source of the weight gradient: NCHW fp32 (N, c, H, W); ab [N][8 ceil(c / 8)][2] or null (untransformed)
struct SegGradSrc {
    const float *x;
    const float *ab;
    int c;
};

constexpr int SEG_WG_K = 16;  // pixels of one contraction step: 16 consecutive pixels of a row

struct SegWgradArgs {
    const float *g;  // (N, cout, H, W)
    SegGradSrc A, B;
    float *part;     // [segments][cout][cin_a + cin_b][KS * KS]
    int *flag;
    int N, H, W, cout;
    int vec;         // W % 4 == 0 and every tensor 16-byte aligned: rows are read with 16-byte loads
    int xs;          // steps per row: ceil(W / 16)
    long steps;      // N H xs
    long per_seg;    // steps of one segment (the last may hold fewer)
};

__device__ __forceinline__ f16x8 seg_pack8(const _Float16 *v) {
    return f16x8{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
}

// grid = (tiles of 32 input channels, tiles of 32 output channels, pixel segments); block = 4 waves.  A step is 16
// consecutive pixels of one row; wave w of a segment takes its steps w, w + 4, ...  MFMA rows are output channels
// (A operand: lane (co, h) holds g at pixels 8h .. 8h+7 of the step), columns are input channels (B operand: lane (ci, h)
// holds v at the same pixels shifted by the tap).  The four waves' accumulators are added in wave order through LDS and
// stored as the segment's partial; seg_wgrad_merge_kernel adds the partials in segment order.
template <int KS>
__global__ void __launch_bounds__(256) seg_wgrad_f16_kernel(const SegWgradArgs p) {
    constexpr int P = KS / 2, NV = 8 + KS - 1, T = KS * KS;
    __shared__ float red[4][1024];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, m = lane & 31;
    const int cin = p.A.c + p.B.c;
    const int ci = 32 * blockIdx.x + m, co = 32 * blockIdx.y + m;
    const int seg = blockIdx.z;

    // this lane's column: a channel of source A, of source B, or a padding column
    const float *vx = nullptr, *vab = nullptr;
    int vc = 0, vch = 0;
    if (ci < p.A.c)
        vx = p.A.x, vab = p.A.ab, vc = p.A.c, vch = ci;
    else if (ci < cin)
        vx = p.B.x, vab = p.B.ab, vc = p.B.c, vch = ci - p.A.c;
    const int vcp = (vc + 7) / 8 * 8;
    const bool gok = co < p.cout;

    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    bool bad = false;

    const long s0 = (long)seg * p.per_seg;
    const long s1 = s0 + p.per_seg < p.steps ? s0 + p.per_seg : p.steps;
    for (long s = s0 + wave; s < s1; s += 4) {  // (uniform per wave)
        const int xi = (int)(s % p.xs);
        const long t_ = s / p.xs;
        const int y = (int)(t_ % p.H), n = (int)(t_ / p.H);
        const int x0 = SEG_WG_K * xi + 8 * h;

        _Float16 ghv[8], glv[8];
        const float *gp = p.g + (((size_t)n * p.cout + (gok ? co : 0)) * p.H + y) * p.W;
        float gv[8];
        if (p.vec) {  // (uniform; W % 4 == 0: a group of four pixels lies inside the row or outside it)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 t = (gok && x0 + 4 * q < p.W) ? *(const f32x4 *)(gp + x0 + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < 4; ++k) gv[4 * q + k] = t[k];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) gv[j] = (gok && x0 + j < p.W) ? gp[x0 + j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bad |= !(__builtin_fabsf(gv[j]) <= F16_MAX);
            split_f16(gv[j], ghv[j], glv[j]);
        }
        const f16x8 gh = seg_pack8(ghv), gl = seg_pack8(glv);

        float a = 1.0f, b = 0.0f;
        if (vab) a = vab[((size_t)n * vcp + vch) * 2], b = vab[((size_t)n * vcp + vch) * 2 + 1];
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const int yy = y + ky - P;
            const bool rowok = vx && yy >= 0 && yy < p.H;
            const float *vp = vx + (((size_t)n * vc + vch) * p.H + (rowok ? yy : 0)) * p.W;
            _Float16 hi[NV], lo[NV];
            float xw[NV];  // the row's window x0 - P .. x0 + 7 + P
            if (p.vec) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const f32x4 t = (rowok && x0 + 4 * q < p.W) ? *(const f32x4 *)(vp + x0 + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int k = 0; k < 4; ++k) xw[P + 4 * q + k] = t[k];
                }
                if (P) {
                    xw[0] = (rowok && x0 >= 1 && x0 - 1 < p.W) ? vp[x0 - 1] : 0.0f;
                    xw[NV - 1] = (rowok && x0 + 8 < p.W) ? vp[x0 + 8] : 0.0f;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int x = x0 + i - P;
                    xw[i] = (rowok && x >= 0 && x < p.W) ? vp[x] : 0.0f;
                }
            }
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int x = x0 + i - P;
                const bool inside = rowok && x >= 0 && x < p.W;
                const float xv = xw[i];
                float v;
                if (vab) {
                    const float t = __builtin_fmaf(a, xv, b);
                    bad |= inside && !(t <= F16_MAX);
                    v = inside ? __builtin_fmaxf(t, 0.0f) : 0.0f;  // zero padding pads v, not x
                } else {
                    bad |= !(__builtin_fabsf(xv) <= F16_MAX);
                    v = xv;
                }
                split_f16(v, hi[i], lo[i]);
            }
#pragma unroll
            for (int kx = 0; kx < KS; ++kx)
                acc[ky * KS + kx] = mfma3(gh, gl, seg_pack8(hi + kx), seg_pack8(lo + kx), acc[ky * KS + kx]);
        }
    }
    if (bad) *p.flag = 1;

#pragma unroll
    for (int t = 0; t < T; ++t) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][r * 64 + lane] = acc[t][r];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, r = e >> 6, l = e & 63;
            const int row = 32 * blockIdx.y + acc_row(r) + 4 * (l >> 5), col = 32 * blockIdx.x + (l & 31);
            const float sum = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
            if (row < p.cout && col < cin) p.part[(((size_t)seg * p.cout + row) * cin + col) * T + t] = sum;
        }
    }
}

// gw[i] = sum over segments, in segment order, in double
static __global__ void seg_wgrad_merge_kernel(const float *part, int segs, size_t total, float *gw) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int k = 0; k < segs; ++k) s += (double)part[(size_t)k * total + i];
        gw[i] = (float)s;
    }
}

// ---- v = relu(GN(x)) backward --------------------------------------------------------------------------------------
__device__ __forceinline__ double seg_block_sum(double *red, double v) {  // 256 threads, fixed tree, all threads get it
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// One block per (sample, channel) plane: mean and rstd recomputed from x in two passes (as seg_plane_moments_kernel), then
// sum g_u and sum g_u xhat with g_u = g_v [fmaf(a, x, b) > 0].  stats [N C][4] doubles: mean, rstd, sum g_u, sum g_u xhat.
static __global__ void __launch_bounds__(256) seg_norm_reduce_kernel(const float *x, const float *ab, const float *gv,
                                                                     int C, int cp, size_t HW, double *stats) {
    __shared__ double red[256];
    const int c = blockIdx.x % C, n = blockIdx.x / C;
    const float *src = x + (size_t)blockIdx.x * HW, *g = gv + (size_t)blockIdx.x * HW;
    const float a = ab[((size_t)n * cp + c) * 2], b = ab[((size_t)n * cp + c) * 2 + 1];
    double s = 0.0;
    for (size_t i = threadIdx.x; i < HW; i += 256) s += (double)src[i];
    const double mean = seg_block_sum(red, s) / (double)HW;
    const float mf = (float)mean;
    double q = 0.0;
    for (size_t i = threadIdx.x; i < HW; i += 256) {
        const float e = src[i] - mf;
        q += (double)(e * e);
    }
    const float var = (float)(seg_block_sum(red, q) / (double)HW);
    const float rstd = 1.0f / __builtin_sqrtf(var + SEG_EPS);
    double sg = 0.0, sgx = 0.0;
    for (size_t i = threadIdx.x; i < HW; i += 256) {
        const float xv = src[i];
        const float gu = __builtin_fmaf(a, xv, b) > 0.0f ? g[i] : 0.0f;
        const float xh = (xv - mf) * rstd;
        sg += (double)gu;
        sgx += (double)gu * (double)xh;
    }
    sg = seg_block_sum(red, sg);
    sgx = seg_block_sum(red, sgx);
    if (threadIdx.x == 0) {
        double *dst = stats + 4 * (size_t)blockIdx.x;
        dst[0] = (double)mf, dst[1] = (double)rstd, dst[2] = sg, dst[3] = sgx;
    }
}

// grid = (N C, blocks per plane).  g_x = gamma rstd (g_u - mean(g_u) - xhat mean(g_u xhat)); the first block of every
// channel's sample-0 plane adds the planes' sums over the samples, in sample order, into dgamma / dbeta.  gx may be null.
static __global__ void __launch_bounds__(256) seg_norm_apply_kernel(const float *x, const float *ab, const float *gamma,
                                                                    const float *gv, const double *stats, int N, int C,
                                                                    int cp, size_t HW, float *gx, float *dgamma,
                                                                    float *dbeta) {
    const int plane = blockIdx.x, c = plane % C, n = plane / C;
    if (n == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        double sb = 0.0, sgm = 0.0;
        for (int k = 0; k < N; ++k) sb += stats[4 * ((size_t)k * C + c) + 2], sgm += stats[4 * ((size_t)k * C + c) + 3];
        dbeta[c] = (float)sb, dgamma[c] = (float)sgm;
    }
    if (!gx) return;
    const double *st = stats + 4 * (size_t)plane;
    const float mf = (float)st[0], rstd = (float)st[1];
    const float mg = (float)(st[2] / (double)HW), mgx = (float)(st[3] / (double)HW);
    const float a = ab[((size_t)n * cp + c) * 2], b = ab[((size_t)n * cp + c) * 2 + 1];
    const float coef = gamma[c] * rstd;
    const float *src = x + (size_t)plane * HW, *g = gv + (size_t)plane * HW;
    float *dst = gx + (size_t)plane * HW;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.y * 256) {
        const float xv = src[i];
        const float gu = __builtin_fmaf(a, xv, b) > 0.0f ? g[i] : 0.0f;
        const float xh = (xv - mf) * rstd;
        dst[i] = coef * __builtin_fmaf(-xh, mgx, gu - mg);
    }
}

// no normalisation (gamma == null): g_x = g_v [fmaf(a, x, b) > 0]
static __global__ void seg_relu_backward_kernel(const float *x, const float *ab, const float *gv, int C, int cp, size_t HW,
                                                size_t total, float *gx) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t plane = i / HW;
        const int c = (int)(plane % C);
        const size_t n = plane / C;
        const float a = ab[(n * cp + c) * 2], b = ab[(n * cp + c) * 2 + 1];
        gx[i] = __builtin_fmaf(a, x[i], b) > 0.0f ? gv[i] : 0.0f;
    }
}

// out[c] = sum over samples and pixels of g (N, C, HW), double accumulators: one block per (sample, channel) plane on a
// fixed tree into part [N][C], then one thread per channel adds the samples in order
static __global__ void __launch_bounds__(256) seg_plane_sums_kernel(const float *g, size_t HW, double *part) {
    __shared__ double red[256];
    const float *src = g + (size_t)blockIdx.x * HW;
    double s = 0.0;
    for (size_t i = threadIdx.x; i < HW; i += 256) s += (double)src[i];
    s = seg_block_sum(red, s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

static __global__ void seg_channel_sums_kernel(const double *part, int N, int C, float *out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += part[(size_t)n * C + c];
    out[c] = (float)s;
}

// ---- device packer ---------------------------------------------------------------------------------------------
// pack_seg_f16 (cae_pack.cpp) on the device: records [group][q][ky][kx][ct] of [hl][lane][8] halves, one thread per value.
// A value outside the f16 range (or NaN) raises *flag.
static __global__ void seg_pack_dev_kernel(const float *w, int cin_a, int cin_b, int cout, int ks, int up, int ct,
                                           int chunks, int m, size_t records, _Float16 *out, int *flag) {
    const int pa = (cin_a + 7) / 8, cp = (cout + 7) / 8 * 8, cin = cin_a + cin_b;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < records * 512; i += (size_t)gridDim.x * blockDim.x) {
        const size_t rec = i >> 9;
        const int lane = (int)(i & 511) >> 3, j = (int)(i & 7);
        size_t t = rec;
        const int r4 = (int)(t % ct);
        t /= ct;
        const int r3 = (int)(t % ks);
        t /= ks;
        const int r2 = (int)(t % ks);
        t /= ks;
        const int r1 = (int)(t % chunks), r0 = (int)(t / chunks);
        const int row = 32 * (r0 * ct + r4) + (lane & 31), k = 16 * r1 + 8 * (lane >> 5) + j;
        int ci = -1;
        if (k < 8 * pa) {
            if (k < cin_a) ci = k;
        } else if (k - 8 * pa < cin_b) {
            ci = cin_a + k - 8 * pa;
        }
        float v = 0.0f;
        if (ci >= 0 && row < m) {
            if (up) {
                const int par = row / cp, co = row % cp;
                if (co < cout) v = w[((size_t)ci * cout + co) * 4 + par];
            } else {
                v = w[(((size_t)row * cin + ci) * ks + r2) * ks + r3];
            }
        }
        bad |= !(__builtin_fabsf(v) <= F16_MAX);
        const _Float16 hi = (_Float16)v;
        out[rec * 1024 + lane * 8 + j] = hi;
        out[rec * 1024 + 512 + lane * 8 + j] = (_Float16)(v - (float)hi);
    }
    if (bad && flag) *flag = 1;
}

// dst[r] = src[up ? r % cp : r] for rows r < m whose channel is real, else 0 (the bias vector seg_conv_f16_kernel reads,
// gamma / beta padded to whole planes); a value outside the f16 range raises *flag when `guard`
static __global__ void seg_pad_vec_kernel(const float *src, int c, int cp, int m, int up, int total, int guard, float *dst,
                                          int *flag) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= total) return;
    const int co = up ? r % cp : r;
    const float v = (r < m && co < c) ? src[co] : 0.0f;
    if (guard && flag && !(__builtin_fabsf(v) <= F16_MAX)) *flag = 1;
    dst[r] = v;
}

}  // namespace cae
