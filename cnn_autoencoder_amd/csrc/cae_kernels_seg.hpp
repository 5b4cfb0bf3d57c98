// Kernels of the segmentation head (JNet on latents and decoder bridges), f16x3 on v_mfma_f32_32x32x16_f16.
//
// Activations between the head's layers are RAW fp32 convolution outputs in C8 rows [N][P][H][W][8].  GroupNorm with
// one group per channel followed by ReLU is an affine map per (sample, channel) and a maximum:
//     v = max(fmaf(a, x, b), 0),   a = gamma rstd,  b = beta - mean a,
// and the CONSUMER applies it while it stages its operand: one fp32 fmaf and one max per value (a host replay
// reproduces v bit for bit), then the split into hi / lo halves on the way into LDS.  The statistics behind (a, b) come
// from the producer's epilogue: per (output tile, sample, channel) a Welford partial over the tile's valid pixels,
// merged in tile order by seg_stats_finalize_kernel.  No atomics: results are bitwise repeatable.
#pragma once
#include "cae_kernels_f16.hpp"

namespace cae {

constexpr int SEG_TX = 16, SEG_TY = 8;  // output tile: 4 waves x (2 rows x 16 pixels)
constexpr float SEG_EPS = 1e-5f;
enum { SEG_OUT_C8 = 0, SEG_OUT_NCHW = 1, SEG_OUT_SHUFFLE = 2 };

// One operand of the contraction: C8 rows and, per (sample, channel of the plane grid), the pair (a, b); ab == null
// stages the values untransformed (raw latents, transposed-convolution outputs: no ReLU either).
struct SegSrc {
    const float *x;
    const float *ab;  // [N][8 planes][2]
    int planes;
};

struct SegConvArgs {
    SegSrc A, B;        // the contraction runs over A's planes, then B's (torch.cat without the copy); B.planes may be 0
    const char *wp;     // pack_seg_f16
    const float *bias;  // [groups * CT * 32] or null
    float *out;
    float *stats;       // [tile][N][8 out_planes][3] Welford partials (count, mean, M2), or null
    int *flag;          // range guard word of the call
    int N, H, W, tiles_x, tiles_y, chunks;
    int cout;        // real output channels (NCHW store)
    int out_planes;  // planes of the C8 output (SHUFFLE: of the 2H x 2W output)
    int outmode;
};

// Chan's merge of two (count, mean, M2) partials, left to right.  The running values are doubles: a partial mean is
// exact to fp32 rounding, and the merged mean must stay accurate relative to |mean|, not to the spread of the tile means
// (planes of zero-mean convolution outputs have |mean| far below sigma).
__device__ __forceinline__ void seg_merge(double &n, double &mean, double &m2, float nb_, float mb_, float m2b_) {
    const double nb = nb_, mb = mb_, m2b = m2b_;
    if (nb == 0.0) return;
    if (n == 0.0) {
        n = nb, mean = mb, m2 = m2b;
        return;
    }
    const double nn = n + nb, d = mb - mean;
    mean = mean + d * (nb / nn);
    m2 = m2 + m2b + d * d * (n * nb / nn);
    n = nn;
}

// (a, b) of GroupNorm(C groups) from a plane's count, mean and M2: biased variance, eps inside the root
__device__ __forceinline__ void seg_affine(double n, double mean_, double m2, float gamma, float beta, float *ab) {
    const float var = n > 0.0 ? (float)(m2 / n) : 0.0f, mean = (float)mean_;
    const float a = gamma * (1.0f / __builtin_sqrtf(var + SEG_EPS));
    ab[0] = a;
    ab[1] = __builtin_fmaf(-mean, a, beta);  // (one rounding, whatever the contraction setting)
}

__device__ __forceinline__ float seg_sum32(float v) {  // over the 32 lanes of a wave half, fixed order, all lanes get it
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ double seg_sum32(double v) {
#pragma unroll
    for (int s = 16; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// =================================================================================================
// seg_conv_f16_kernel: stride-1 zero-padded KS x KS convolution over two sources, CT channel tiles per block,
//   blockIdx.y = group of CT tiles.  Block = 4 waves, tile = 8 x 16 output pixels; stage = one 16-channel chunk:
//     weights [ky][kx][ct][hl][64][8 f16]   +   halo [pl][hl][HH rows][WH][16 B]
//   Both operands are staged through registers (the activation transform forces it, and mixing LDS-DMA with ordinary
//   loads in one k-loop would drain with vmcnt(0)): one register set, chunk t+1 is written into the other LDS buffer
//   after the barrier, the loads of chunk t+2 are issued at once and land under chunk t's MFMAs.
// =================================================================================================
template <int KS, int CT>
struct SegGeom {
    static constexpr int PAD = KS / 2, HH = SEG_TY + KS - 1, WH = SEG_TX + KS - 1, NPX = HH * WH;
    static constexpr int HALO_BYTES = 4 * NPX * 16;
    static constexpr int W_PIECES = KS * KS * CT * 128;
    static constexpr int W_BYTES = W_PIECES * 16;
    static constexpr int W_PER = (W_PIECES + 255) / 256;
    static constexpr int STAGE_BYTES = W_BYTES + HALO_BYTES;
    static constexpr int RED_BYTES = 4 * CT * 32 * 3 * 4;
    static constexpr int LDS_BYTES = 2 * STAGE_BYTES > RED_BYTES ? 2 * STAGE_BYTES : RED_BYTES;
};

template <int KS, int CT>
__global__ void __launch_bounds__(256) seg_conv_f16_kernel(const SegConvArgs p) {
    using G = SegGeom<KS, CT>;
    constexpr int WH = G::WH, NPX = G::NPX, W_BYTES = G::W_BYTES, W_PIECES = G::W_PIECES, W_PER = G::W_PER;
    static_assert(NPX <= 256, "one halo pixel per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, m = lane & 31;
    int bid = blockIdx.x;
    const int tile = bid % (p.tiles_x * p.tiles_y);
    const int tx = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int n = bid / p.tiles_y;
    const int grp = blockIdx.y;
    const int oy0 = ty * SEG_TY, ox0 = tx * SEG_TX;
    const size_t HW = (size_t)p.H * p.W;

    // this thread's halo pixel (threads NPX .. 255 have none)
    const int hr = tid / WH, hx = tid - hr * WH;
    const int iy = oy0 - G::PAD + hr, ix = ox0 - G::PAD + hx;
    const bool inside = tid < NPX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    const size_t pix = inside ? (size_t)iy * p.W + ix : 0;
    const int planes = p.A.planes + p.B.planes;

    f32x4 raw[2][2];
    u32x4v wreg[W_PER];
    const char *wsrc = p.wp + (size_t)grp * p.chunks * W_BYTES;
    bool bad = false;

    auto load = [&](int q) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const int g = 2 * q + pl;  // (uniform) plane of the concatenated grid
            const float *src = nullptr;
            if (g < p.A.planes)
                src = p.A.x + ((size_t)n * p.A.planes + g) * HW * 8;
            else if (g < planes)
                src = p.B.x + ((size_t)n * p.B.planes + (g - p.A.planes)) * HW * 8;
            raw[pl][0] = raw[pl][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (src && inside) {
                raw[pl][0] = *(const f32x4 *)(src + pix * 8);
                raw[pl][1] = *(const f32x4 *)(src + pix * 8 + 4);
            }
        }
#pragma unroll
        for (int i = 0; i < W_PER; ++i) {
            const int idx = tid + i * 256;
            if (idx < W_PIECES) wreg[i] = *(const u32x4v *)(wsrc + (size_t)q * W_BYTES + (size_t)idx * 16);
        }
    };
    auto commit = [&](int q, char *buf) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const int g = 2 * q + pl;
            const float *ab = nullptr;  // (uniform: scalar loads)
            if (g < p.A.planes) {
                if (p.A.ab) ab = p.A.ab + ((size_t)n * p.A.planes + g) * 16;
            } else if (g < planes) {
                if (p.B.ab) ab = p.B.ab + ((size_t)n * p.B.planes + (g - p.A.planes)) * 16;
            }
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float x = raw[pl][k >> 2][k & 3];
                if (ab) {
                    const float t = __builtin_fmaf(ab[2 * k], x, ab[2 * k + 1]);
                    bad |= inside && !(t <= F16_MAX);  // (negated compare: a NaN raises too; below zero the ReLU clamps)
                    v[k] = inside ? __builtin_fmaxf(t, 0.0f) : 0.0f;  // zero padding pads v, not x
                } else {
                    bad |= !(__builtin_fabsf(x) <= F16_MAX);
                    v[k] = x;
                }
            }
            u32x4v hi, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const u32x2v t_ = split2_f16(v[2 * e], v[2 * e + 1]);
                hi[e] = t_[0];
                lo[e] = t_[1];
            }
            if (tid < NPX) {
                *(u32x4v *)(buf + W_BYTES + ((pl * 2 + 0) * NPX + tid) * 16) = hi;
                *(u32x4v *)(buf + W_BYTES + ((pl * 2 + 1) * NPX + tid) * 16) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < W_PER; ++i) {
            const int idx = tid + i * 256;
            if (idx < W_PIECES) *(u32x4v *)(buf + idx * 16) = wreg[i];
        }
    };

    f32x16 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[ct][r] = p.bias ? p.bias[32 * (grp * CT + ct) + acc_row(r) + 4 * h] : 0.0f;

    // B operand of tap (ky, kx): halo [pl = h][hl][row 2 wave + (m>>4) + ky][(m&15) + kx]
    const int b_off = W_BYTES + ((2 * h) * NPX + (2 * wave + (m >> 4)) * WH + (m & 15)) * 16;
    constexpr int B_HL = NPX * 16;

    load(0);
    commit(0, smem);
    if (p.chunks > 1) load(1);
    for (int t = 0; t < p.chunks; ++t) {
        __syncthreads();
        const char *cur = smem + (t & 1) * G::STAGE_BYTES;
        if (t + 1 < p.chunks) commit(t + 1, smem + ((t + 1) & 1) * G::STAGE_BYTES);
        if (t + 2 < p.chunks) load(t + 2);
        const char *wb = cur + lane * 16, *hb = cur + b_off;
#pragma unroll
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const f16x8 bh = *(const f16x8 *)(hb + (ky * WH + kx) * 16);
                const f16x8 bl = *(const f16x8 *)(hb + (ky * WH + kx) * 16 + B_HL);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const f16x8 ah = *(const f16x8 *)(wb + (((ky * KS + kx) * CT + ct) * 2 + 0) * 1024);
                    const f16x8 al = *(const f16x8 *)(wb + (((ky * KS + kx) * CT + ct) * 2 + 1) * 1024);
                    acc[ct] = mfma3(ah, al, bh, bl, acc[ct]);
                }
            }
    }
    if (bad) *p.flag = 1;

    const int oy = oy0 + 2 * wave + (m >> 4), ox = ox0 + (m & 15);
    const bool valid = oy < p.H && ox < p.W;
    // lane (pixel, h) holds channels 4h .. 4h+3 of plane 4 (grp CT + ct) + (r >> 2) in acc[ct][4 (r >> 2) ..]
    if (valid) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int plane = 4 * (grp * CT + ct) + g;  // (uniform)
                const f32x4 v = {acc[ct][4 * g], acc[ct][4 * g + 1], acc[ct][4 * g + 2], acc[ct][4 * g + 3]};
                if (p.outmode == SEG_OUT_C8) {
                    if (plane < p.out_planes)
                        *(f32x4 *)(p.out + (((size_t)n * p.out_planes + plane) * HW + (size_t)oy * p.W + ox) * 8 + 4 * h) = v;
                } else if (p.outmode == SEG_OUT_SHUFFLE) {
                    // row = (2 dy + dx) CP + co: plane = par out_planes + output plane
                    const int par = plane / p.out_planes, op = plane - par * p.out_planes;
                    if (par < 4) {
                        const size_t o = ((size_t)n * p.out_planes + op) * (4 * HW) +
                                         (size_t)(2 * oy + (par >> 1)) * (2 * p.W) + (2 * ox + (par & 1));
                        *(f32x4 *)(p.out + o * 8 + 4 * h) = v;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = 8 * plane + 4 * h + k;
                        if (c < p.cout) p.out[((size_t)n * p.cout + c) * HW + (size_t)oy * p.W + ox] = v[k];
                    }
                }
            }
    }

    if (p.stats) {  // (uniform)
        float *red = (float *)smem;  // [wave][CT * 32][3]
        __syncthreads();             // every wave is through with the staging buffers
        const float cnt = seg_sum32(valid ? 1.0f : 0.0f);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // two passes over the wave's 32 pixels: the sum in double (exact to 2^-53, so the mean is the rounded exact
                // mean: a one-pixel plane gives mean == x and M2 == 0, a large mean costs the deviations no bits), then
                // the squared deviations from it in fp32
                const float x = acc[ct][r];
                const double s = seg_sum32(valid ? (double)x : 0.0);
                const float mean = cnt > 0.0f ? (float)(s / (double)cnt) : 0.0f;
                const float e = valid ? x - mean : 0.0f;
                const float m2 = seg_sum32(e * e);
                if (m == 0) {
                    float *dst = red + (wave * CT * 32 + 32 * ct + acc_row(r) + 4 * h) * 3;
                    dst[0] = cnt, dst[1] = mean, dst[2] = m2;
                }
            }
        __syncthreads();
        const int c = 32 * grp * CT + tid;
        if (tid < CT * 32 && c < 8 * p.out_planes) {
            double cn = 0.0, mean = 0.0, m2 = 0.0;
            for (int w = 0; w < 4; ++w) {
                const float *src = red + (w * CT * 32 + tid) * 3;
                seg_merge(cn, mean, m2, src[0], src[1], src[2]);
            }
            float *dst = p.stats + (((size_t)tile * p.N + n) * (8 * p.out_planes) + c) * 3;
            dst[0] = (float)cn, dst[1] = (float)mean, dst[2] = (float)m2;
        }
    }
}

// Merges the tile partials of every (sample, channel) plane in tile order and writes (a, b).  gamma == null (the head
// was built without normalisation): the identity (1, 0), the consumer's ReLU still applies.
static __global__ void seg_stats_finalize_kernel(const float *stats, int tiles, int N, int cp, const float *gamma,
                                                 const float *beta, float *ab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // n * cp + c
    if (i >= N * cp) return;
    if (!gamma) {
        ab[2 * i] = 1.0f, ab[2 * i + 1] = 0.0f;
        return;
    }
    double cn = 0.0, mean = 0.0, m2 = 0.0;
    for (int t = 0; t < tiles; ++t) {
        const float *src = stats + ((size_t)t * N * cp + i) * 3;
        seg_merge(cn, mean, m2, src[0], src[1], src[2]);
    }
    seg_affine(cn, mean, m2, gamma[i % cp], beta[i % cp], ab + 2 * i);
}

// (a, b) of the planes of an NCHW fp32 tensor no kernel of this file produced (the bridges entering the projection
// unit): one block per (sample, channel of the plane grid), two passes (sum, then squared deviations), double
// accumulators, fixed tree order.
static __global__ void __launch_bounds__(256) seg_plane_moments_kernel(const float *x, int C, int cp, size_t HW,
                                                                       const float *gamma, const float *beta, float *ab) {
    __shared__ double red[256];
    const int c = blockIdx.x % cp, n = blockIdx.x / cp;
    float *dst = ab + 2 * (size_t)blockIdx.x;
    if (c >= C || !gamma) {  // padding channel / no normalisation
        if (threadIdx.x == 0) dst[0] = gamma ? 0.0f : 1.0f, dst[1] = 0.0f;
        return;
    }
    const float *src = x + ((size_t)n * C + c) * HW;
    auto block_sum = [&](double v) {
        __syncthreads();
        red[threadIdx.x] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        return red[0];
    };
    double s = 0.0;
    for (size_t i = threadIdx.x; i < HW; i += 256) s += (double)src[i];
    const double mean = block_sum(s) / (double)HW;
    const float mf = (float)mean;
    double q = 0.0;
    for (size_t i = threadIdx.x; i < HW; i += 256) {
        const float e = src[i] - mf;
        q += (double)(e * e);
    }
    const double m2 = block_sum(q);
    if (threadIdx.x == 0) seg_affine((double)HW, mean, m2, gamma[c], beta[c], dst);
}

}  // namespace cae
