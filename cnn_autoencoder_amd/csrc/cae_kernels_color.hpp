// Colour layer of a synthesis level to at most 4 image channels (the multiscale colour layers, _autoencoders.py:417-436):
// nn.Conv2d(k, stride 1, padding k//2, padding_mode='reflect') (+ bias) of a level's activations, with the fp32 NCHW or
// the uint8 HWC epilogue (:576-580) -- the last kernel of a synthesis that stops at a level (cae_synthesis_scale).
//
// Why not the generic stride-1 launch: the MFMA tiles are 32 (fp32) / 32 (f16x3) output channels wide, so a 3-channel
// image costs 10.7 times its MACs there.  With <= 4 output channels no matrix shape fits better: the smallest fp32
// shapes (16x16x4, 4x4x1 x 16 blocks) run at the rate of the vector FMA (64 FLOP / clk / SIMD either way) and leave
// 12 of 16 columns empty or add nothing; so the contraction is plain fp32 FMA on the vector unit, 4 channels x 4 pixels
// of accumulators per lane, and computes the useful MACs only.
//
//   block  = 4 waves, tile = 64 x 16 output pixels; lane l of wave w owns column l, rows 4w .. 4w+3
//   stage  = one 8-channel plane of the (16 + k - 1) x (64 + k - 1) reflect halo, fp32 in LDS as two float4 images
//            [channels 0-3][channels 4-7] (16-byte pixels: consecutive lanes read consecutive slots, no bank conflict)
//   x      : per kernel column one ds_read_b128 pair per halo row (4 + k - 1 rows) feeds k rows x 4 pixels x 8 channels
//            x 4 outputs = 128 k FMAs (k = 3: 32 FMAs per 16-byte read)
//   w      : [chunk][ky][kx][8 channels][4 outputs] fp32, addressed by loop counters only: wave-uniform scalar loads
//   SPLIT  : the level is stored as C8SP rows (f16x3 path); hi + lo is formed in fp32 while staging -- exactly the value
//            the split format carries (cae_kernels_f16.hpp: |v - (hi + lo)| <= max(2^-22 |v|, 2^-25)) -- and the
//            products are fp32 x fp32 with fp32 weights: inside the f16x3 contract (no dropped lo x lo term).  A result
//            that is not finite raises the call's range flag, like every kernel of that path.
#pragma once
#include "cae_kernels_f16.hpp"

namespace cae {

struct ColorArgs {
    const void *in;     // C8 fp32 [N][in_planes][H][W][8] | C8SP rows
    void *out;          // NCHW float | HWC uint8
    const float *w;     // [chunks][KS][KS][8][4], zero padded
    const float *bias;  // [4] (zero padded) or nullptr
    int N, H, W;
    int in_planes;      // plane stride of the input buffer
    int chunks;         // 8-channel planes contracted
    int cout;           // image channels (1 .. 4)
    int tiles_x, tiles_y;
    int outfmt;         // OUT_NCHW | OUT_U8HWC
    int *flag;          // SPLIT: range flag of the call
};

constexpr int COLOR_TX = 64, COLOR_TY = 16, COLOR_NW = 4, COLOR_PY = COLOR_TY / COLOR_NW;

template <int KS>
constexpr int color_lds_bytes() {
    return (COLOR_TY + KS - 1) * (COLOR_TX + KS - 1) * 32;
}

template <int KS, bool SPLIT>
__global__ void __launch_bounds__(COLOR_NW * 64, 2) color_small_kernel(const ColorArgs p) {
    constexpr int PAD = KS / 2;
    constexpr int HR = COLOR_TY + KS - 1, HC = COLOR_TX + KS - 1;  // halo rows / columns
    constexpr int NR = COLOR_PY + KS - 1;                          // halo rows under one lane's 4 pixels
    __shared__ f32x4 halo[2][HR][HC];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int n = bid / p.tiles_y;
    const int x0 = tx * COLOR_TX, y0 = ty * COLOR_TY;

    float acc[COLOR_PY][4];
#pragma unroll
    for (int j = 0; j < COLOR_PY; ++j)
#pragma unroll
        for (int co = 0; co < 4; ++co) acc[j][co] = p.bias ? p.bias[co] : 0.0f;

    const size_t row_bytes = SPLIT ? c8s_row_bytes<true>(p.W) : (size_t)p.W * 32;
    for (int c = 0; c < p.chunks; ++c) {
        const char *plane = (const char *)p.in + ((size_t)n * p.in_planes + c) * p.H * row_bytes;
        __syncthreads();  // the previous plane's reads are done
        for (int i = threadIdx.x; i < HR * HC; i += COLOR_NW * 64) {
            const int r = i / HC, q = i - r * HC;
            // reflect_idx clamps: a halo pixel of a tile that overhangs the image reads some pixel inside it (unused)
            const int sy = reflect_idx(y0 - PAD + r, p.H), sx = reflect_idx(x0 - PAD + q, p.W);
            f32x4 a, b;
            if constexpr (SPLIT) {
                const char *src = plane + (size_t)sy * row_bytes + c8s_piece<true>(sx);
                const f16x8 vh = *(const f16x8 *)src, vl = *(const f16x8 *)(src + 512);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = (float)vh[k] + (float)vl[k];
                    b[k] = (float)vh[4 + k] + (float)vl[4 + k];
                }
            } else {
                const float *src = (const float *)(plane + (size_t)sy * row_bytes) + (size_t)sx * 8;
                a = *(const f32x4 *)src;
                b = *(const f32x4 *)(src + 4);
            }
            halo[0][r][q] = a;
            halo[1][r][q] = b;
        }
        __syncthreads();
        const float *wc = p.w + (size_t)c * KS * KS * 32;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            f32x4 xa[NR], xb[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                xa[r] = halo[0][wave * COLOR_PY + r][lane + kx];
                xb[r] = halo[1][wave * COLOR_PY + r][lane + kx];
            }
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
                const float *wk = wc + (ky * KS + kx) * 32;
#pragma unroll
                for (int ch = 0; ch < 8; ++ch) {
                    const f32x4 wv = *(const f32x4 *)(wk + ch * 4);
#pragma unroll
                    for (int j = 0; j < COLOR_PY; ++j) {
                        const float xv = ch < 4 ? xa[j + ky][ch] : xb[j + ky][ch - 4];
#pragma unroll
                        for (int co = 0; co < 4; ++co) acc[j][co] = __builtin_fmaf(xv, wv[co], acc[j][co]);
                    }
                }
            }
        }
    }

    const int ox = x0 + lane;
    if (ox >= p.W) return;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < COLOR_PY; ++j) {
        const int oy = y0 + wave * COLOR_PY + j;
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            if (oy < p.H && co < p.cout) {
                const float v = acc[j][co];
                if constexpr (SPLIT) bad |= !(__builtin_fabsf(v) <= 3.4028234664e38f);
                if (p.outfmt == OUT_U8HWC)  // x*255 -> clip(0,255) -> truncating cast  (_autoencoders.py:576-580)
                    ((uint8_t *)p.out)[(((size_t)n * p.H + oy) * p.W + ox) * p.cout + co] = clip_u8(v * 255.0f);
                else
                    ((float *)p.out)[(((size_t)n * p.cout + co) * p.H + oy) * p.W + ox] = v;
            }
        }
    }
    if constexpr (SPLIT) {
        if (bad) *p.flag = 1;
    }
}

// fp32 NCHW -> uint8 HWC with the image epilogue (colour layers the small kernel does not cover: more than 128 input
// or 4 image channels go through the generic launch, which writes fp32 NCHW only)
static __global__ void nchw_to_u8hwc_kernel(const float *in, uint8_t *out, int N, int C, size_t HW) {
    const size_t total = (size_t)N * HW * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t np = i / C;
        const size_t pix = np % HW, n = np / HW;
        out[i] = clip_u8(in[(n * C + c) * HW + pix] * 255.0f);
    }
}

}  // namespace cae
