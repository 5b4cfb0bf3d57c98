// C ABI of the training path (include/cae_hip.h, "training"): stateless launches on caller-owned device buffers.
// The launch decisions of the MFMA kernels -- taps, halo, LDS, kernel, grid -- are each made once, in the helpers of the
// anonymous namespace; tests/native/train_launches.cpp records what every entry point launches, without a GPU.
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"
#include "cae_train_kernels.hpp"
#include "cae_train_gdn.hpp"

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>

using namespace cae;
using namespace cae::tr;

namespace {

std::atomic<int> g_samples_per_block{0};  // cae_t_set_samples_per_block (0: automatic)

// 1 KiB of zeros on the current device (the halo source of positions outside the input), or null
const void *zero_page() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    static std::map<int, void *> pages;
    std::lock_guard<std::mutex> lock(launch_mutex());
    void *&z = pages[dev];
    if (!z) {
        void *p = nullptr;
        if (hipMalloc(&p, 1024) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, 1024) != hipSuccess) {
            (void)hipFree(p);
            return nullptr;
        }
        z = p;
    }
    return z;
}

unsigned ew_grid(size_t total) {
    const size_t b = (total + 255) / 256;
    return (unsigned)std::min<size_t>(std::max<size_t>(b, 1), TRAIN_CUS * 8 * 4);
}

// raises the kernel's dynamic LDS limit where it asks for LDS, launches it, -> CAE_*
template <class... P, class... A>
int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
    if (lds > 0) CAE_TRY(ensure_lds((const void *)kern, (int)lds));
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// an element-wise kernel: blocks of 256 threads striding over `total` elements
template <class... P, class... A>
int launch_ew(void (*kern)(P...), size_t total, void *stream, A... args) {
    return launch(kern, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, args...);
}

bool bad_channels(int c) { return c < 32 || c % 32 != 0 || c > 32 * MAX_CT; }

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ceil(2^32 / d): __umulhi(x, .) is the exact quotient x / d of the piece indices the kernels divide
unsigned recip32(int d) { return (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }

// f(std::integral_constant<int, CT>) for the run-time tile count ct = 1 .. N (N for anything above)
template <int N, class F>
int for_tiles(int ct, F f) {
    if constexpr (N > 1)
        if (ct < N) return for_tiles<N - 1>(ct, f);
    return f(std::integral_constant<int, N>());
}

// ---- taps ----
struct TapList {
    int n = 0;
    short dy[MAX_TAPS] = {}, dx[MAX_TAPS] = {}, wt[MAX_TAPS] = {};  // input offset and weight index (ky * k + kx) per tap
};

// Appends the taps (ky, kx) of a k x k window whose offsets (oy + s ky, ox + s kx) are multiples of `step`, with
// offset / step.  step 1: the whole window -- o = -P, s = 1: d = k - P;  o = 0, s = -1: d = -k;  o = P, s = -1: d = P - k.
// step 2, s = -1, o = parity + shift: the taps of one output parity of the stride-2 transpose, d = (parity + shift - k) / 2.
void add_taps(TapList &t, int ks, int oy, int ox, int s, int step) {
    for (int ky = 0; ky < ks; ++ky) {
        if ((oy + s * ky) % step != 0) continue;
        for (int kx = 0; kx < ks; ++kx) {
            if ((ox + s * kx) % step != 0) continue;
            t.dy[t.n] = (short)((oy + s * ky) / step);
            t.dx[t.n] = (short)((ox + s * kx) / step);
            t.wt[t.n] = (short)(ky * ks + kx);
            ++t.n;
        }
    }
}

void set_taps(GGArgs &a, const TapList &t) {
    a.ntaps = t.n;
    std::copy(t.dy, t.dy + MAX_TAPS, a.dy);
    std::copy(t.dx, t.dx + MAX_TAPS, a.dx);
    std::copy(t.wt, t.wt + MAX_TAPS, a.wt);
}

// ---- halo ----
// logical positions per tile: 16 x 16 in gather_gemm / gg8 / gg8t (i0 = ty * 16, j0 = tx * 16 there), 8 x 16 in wgrad / wgrad8
constexpr int GG_TILE = 16, WG_TILE_ROWS = 8, WG_TILE_COLS = 16;

// Bounding box of the input pixels a tile of rows x cols positions (stride S apart) reads through the taps, into the
// dymin / dxmin / HR / HC / m_hc of a GGArgs or WGArgs.
template <class Args>
void set_halo(Args &a, const TapList &t, int S, int rows, int cols) {
    int dymin = t.dy[0], dymax = t.dy[0], dxmin = t.dx[0], dxmax = t.dx[0];
    for (int i = 1; i < t.n; ++i) {
        dymin = std::min<int>(dymin, t.dy[i]);
        dymax = std::max<int>(dymax, t.dy[i]);
        dxmin = std::min<int>(dxmin, t.dx[i]);
        dxmax = std::max<int>(dxmax, t.dx[i]);
    }
    a.dymin = dymin;
    a.dxmin = dxmin;
    a.HR = S * (rows - 1) + (dymax - dymin) + 1;
    a.HC = S * (cols - 1) + (dxmax - dxmin) + 1;
    a.m_hc = recip32(a.HC);
}

// ---- LDS ----
// LDS-DMA instructions (1 KiB each) of a halo of nq 8-channel quarters
int halo_instr(int nq, int HR, int HC) { return (nq * HR * HC + 63) / 64; }

// bytes of one staged slice: the halo of nq quarters + the weights of every tap, NT n-tiles, nq / 2 k-steps (1 KiB each)
size_t slice_bytes(int nq, int HR, int HC, int ntaps, int NT) {
    return ((size_t)halo_instr(nq, HR, HC) + (size_t)ntaps * NT * (nq / 2)) * 1024;
}

// quarters per slice of the pipelined form (a slice twice in the LDS): 4 = a 32-channel chunk, 2 = half, 0 = does not fit
int pick_nq(int HR, int HC, int ntaps, int NT, int max_halo_instr) {
    for (int nq : {4, 2})
        if (2 * slice_bytes(nq, HR, HC, ntaps, NT) <= LDS_BUDGET && halo_instr(nq, HR, HC) <= max_halo_instr) return nq;
    return 0;
}

// samples a block of the 8-wave kernels walks: enough blocks for two rounds over the CUs, the rest of the batch amortises
// a block's prologue
int samples_per_block(int n, size_t blocks_per_sample) {
    return (int)std::min<size_t>(std::max<size_t>((size_t)n * blocks_per_sample / (2 * TRAIN_CUS), 1), (size_t)n);
}

// ---- gather-GEMM launches ----
// the tile grid over the logical positions, and the zero page
int set_tiles(GGArgs &a) {
    a.tiles_x = ceil_div(a.LW, GG_TILE);
    a.tiles_y = ceil_div(a.LH, GG_TILE);
    a.zero = zero_page();
    return a.zero ? CAE_OK : fail(CAE_ERR_NOMEM, "zero page");
}

template <int NT, bool PIPE>
int launch_gg_tp(const GGArgs &a, size_t lds, hipStream_t st) {
    const unsigned grid = (unsigned)((size_t)a.N * a.tiles_x * a.tiles_y);
    return launch(gather_gemm_kernel<NT, PIPE>, dim3(grid), dim3(256), lds, st, a);
}

// gg8_kernel (two waves per SIMD, compile-time taps, blocks walking several samples): the shapes of the canonical model
template <int NT, int NQ, int NTAPS>
int launch_gg8(GGArgs a, hipStream_t st) {
    const size_t tiles = (size_t)a.tiles_x * a.tiles_y;
    const int forced = g_samples_per_block.load(std::memory_order_relaxed);
    a.npb = forced > 0 ? std::min(forced, a.N) : samples_per_block(a.N, tiles);
    const unsigned grid = (unsigned)(tiles * (size_t)ceil_div(a.N, a.npb));
    return launch(gg8_kernel<NT, NQ, NTAPS>, dim3(grid), dim3(512), 2 * slice_bytes(NQ, a.HR, a.HC, NTAPS, NT), st, a);
}

// all four output parities of the k = 3 transpose in one launch (gg8t_kernel): 64 output channels per block
template <bool EXT>
int launch_gg8t(GGArgs a, hipStream_t st) {
    const size_t tiles = (size_t)a.tiles_x * a.tiles_y, halves = (size_t)a.Cn / 64;
    a.npb = samples_per_block(a.N, tiles * halves);
    const unsigned grid = (unsigned)(tiles * (size_t)ceil_div(a.N, a.npb));
    return launch(gg8t_kernel<EXT>, dim3(grid, (unsigned)halves), dim3(512), 2 * slice_bytes(4, a.HR, a.HC, 9, 2), st, a);
}

// The gg8_kernel instantiations that are built: n-tiles per launch, quarters per slice, taps, and the launches the
// output's n-tiles are split over (192 output channels go as two launches of three n-tiles: six do not leave room for
// two slice buffers in the LDS).
struct GG8Form {
    int nt, nq, ntaps, parts;
    int (*launch)(GGArgs, hipStream_t);
};
#define GG8_FORM(NT, NQ, NTAPS, PARTS) {NT, NQ, NTAPS, PARTS, launch_gg8<NT, NQ, NTAPS>}
const GG8Form GG8_FORMS[] = {GG8_FORM(3, 2, 9, 2), GG8_FORM(3, 4, 4, 2), GG8_FORM(3, 4, 2, 2), GG8_FORM(3, 4, 1, 2),
                             GG8_FORM(4, 2, 9, 1), GG8_FORM(4, 4, 4, 1), GG8_FORM(4, 4, 2, 1), GG8_FORM(4, 4, 1, 1),
                             GG8_FORM(1, 4, 1, 1)};
#undef GG8_FORM

// the gg8 form that covers a launch whose halo is filled in, or null: gather_gemm_kernel<Cn / 32, nq != 0> runs
const GG8Form *choose_gg8(const GGArgs &a) {
    const int parts = a.Cn / 32 == MAX_CT ? 2 : 1, nt = a.Cn / 32 / parts;
    const int nq = parts == 1 ? a.nq : pick_nq(a.HR, a.HC, a.ntaps, nt, GG8_HALO_INSTR);
    if (nq == 0 || halo_instr(nq, a.HR, a.HC) > GG8_HALO_INSTR) return nullptr;
    for (const GG8Form &f : GG8_FORMS)
        if (f.nt == nt && f.nq == nq && f.ntaps == a.ntaps && f.parts == parts) return &f;
    return nullptr;
}

// fills the taps and the halo / staging geometry of `a`, picks the kernel and launches
int launch_gg(GGArgs &a, const TapList &t, hipStream_t st) {
    if (bad_channels(a.Ck) || bad_channels(a.Cn)) return fail(CAE_ERR_ARG, "channel counts must be multiples of 32, at most 192");
    if (t.n < 1 || t.n > MAX_TAPS) return fail(CAE_ERR_ARG, "bad tap count");
    set_taps(a, t);
    set_halo(a, t, a.S, GG_TILE, GG_TILE);
    const int NT = a.Cn / 32;
    if (halo_instr(4, a.HR, a.HC) > GG_HALO_INSTR) return fail(CAE_ERR_UNSUPPORTED, "halo too large");
    // unpipelined form: the halo of a 32-channel chunk + the weights (2 KiB per tap and n-tile) of as many taps as fit
    const size_t halo = (size_t)halo_instr(4, a.HR, a.HC) * 1024;
    a.taps_per_stage = std::min<int>(a.ntaps, (int)((LDS_BUDGET - halo) / ((size_t)NT * 2048)));
    if (a.taps_per_stage < 1) return fail(CAE_ERR_UNSUPPORTED, "weights of one tap do not fit the LDS");
    a.nq = pick_nq(a.HR, a.HC, a.ntaps, NT, GG_HALO_INSTR);
    const size_t lds = a.nq ? 2 * slice_bytes(a.nq, a.HR, a.HC, a.ntaps, NT) : halo + (size_t)a.taps_per_stage * NT * 2048;
    a.m_plane = recip32(a.HR * a.HC);
    CAE_TRY(set_tiles(a));
    if (const GG8Form *f = choose_gg8(a)) {
        for (int part = 0; part < f->parts; ++part) {
            GGArgs b = a;
            if (f->parts > 1) {
                b.nq = f->nq;
                b.nt0 = f->nt * part;
                b.nt_all = NT;
            }
            CAE_TRY(f->launch(b, st));
        }
        return CAE_OK;
    }
    return for_tiles<MAX_CT>(NT, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        return a.nq ? launch_gg_tp<CT, true>(a, lds, st) : launch_gg_tp<CT, false>(a, lds, st);
    });
}

// operands, shapes, strides and activation of a gather-GEMM launch; the rest of the fields zero
GGArgs gg_args(const void *in16, int n, int ih, int iw, int ck, const void *packed, float *out32, void *out16, int cn, int oh,
               int ow, const float *bias, int S, int SO, int act) {
    GGArgs a{};
    a.in = in16;
    a.out32 = out32;
    a.out16 = out16;
    a.wp = packed;
    a.bias = bias;
    a.N = n;
    a.IH = ih;
    a.IW = iw;
    a.Ck = ck;
    a.Cn = cn;
    a.OH = oh;
    a.OW = ow;
    a.S = S;
    a.SO = SO;
    a.act = act;
    return a;
}

bool bad_kernel_size(int ks) { return ks != 3 && ks != 5; }
int kernel_size_error(int ks) { return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks); }

// Correlation over the whole k x k window, one output pixel per position: position (i, j) <- input (S i + d_ky, S j + d_kx)
// with d_k = o + s k (add_taps).  k = 1: the pointwise product.
int window_corr(GGArgs a, int ks, int o, int s, hipStream_t st) {
    a.LH = a.OH;
    a.LW = a.OW;
    a.ktaps = ks * ks;
    TapList t;
    add_taps(t, ks, o, o, s, 1);
    return launch_gg(a, t, st);
}

// strided correlation: position (i, j) <- input (2i + ky - P, 2j + kx - P), every tap
int strided_corr(const void *in16, int n, int ih, int iw, int ck, const void *packed, int ks, int reflect, float *out32,
                 void *out16, int cn, int oh, int ow, const float *bias, int act, hipStream_t st) {
    if (bad_kernel_size(ks)) return kernel_size_error(ks);
    GGArgs a = gg_args(in16, n, ih, iw, ck, packed, out32, out16, cn, oh, ow, bias, 2, 1, act);
    a.reflect = reflect;
    return window_corr(a, ks, -(ks / 2), 1, st);
}

// transpose of the strided correlation.
//   shift = P : cropped domain   out[Y] = sum in[(Y + P - ky) / 2]  (ConvTranspose2d(k, 2, k//2, output_padding 1))
//   shift = 0 : extended domain  out[Y] = sum in[(Y - ky) / 2],  Y in [0, 2 ih + k - 2]   (data gradient of a valid
//               convolution on the reflect-padded input; Y = y + P)
// k = 3 and a multiple of 64 output channels: all four output parities in one gg8t launch, their tap lists one after the
// other in gg8t_parity's order (0,0), (0,1), (1,0), (1,1); else one launch per output parity.
int strided_corr_t(const void *in16, int n, int ih, int iw, int ck, const void *packed, int ks, int shift, float *out32,
                   void *out16, int cn, int oh, int ow, const float *bias, int act, hipStream_t st) {
    if (bad_kernel_size(ks)) return kernel_size_error(ks);
    GGArgs base = gg_args(in16, n, ih, iw, ck, packed, out32, out16, cn, oh, ow, bias, 1, 2, act);
    base.ktaps = ks * ks;
    if (ks == 3 && (shift == 0 || shift == 1) && cn % 64 == 0 && !bad_channels(ck) && !bad_channels(cn)) {
        GGArgs a = base;
        TapList t;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) add_taps(t, ks, py + shift, px + shift, -1, 2);
        set_taps(a, t);
        set_halo(a, t, 1, GG_TILE, GG_TILE);
        if (halo_instr(4, a.HR, a.HC) <= GG8T_HALO_INSTR) {
            a.LH = (oh + 1) / 2;
            a.LW = (ow + 1) / 2;
            CAE_TRY(set_tiles(a));
            return shift == 0 ? launch_gg8t<true>(a, st) : launch_gg8t<false>(a, st);
        }
    }
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            GGArgs a = base;
            a.LH = (oh - py + 1) / 2;
            a.LW = (ow - px + 1) / 2;
            a.oy0 = py;
            a.ox0 = px;
            TapList t;
            add_taps(t, ks, py + shift, px + shift, -1, 2);
            if (a.LH < 1 || a.LW < 1 || t.n == 0) continue;
            CAE_TRY(launch_gg(a, t, st));
        }
    return CAE_OK;
}

// stride-1 correlations of the LeakyReLU / ReLU units' pre-convolutions: position (i, j) <- input (i + d_ky, j + d_kx)
//   mode 0  analysis pre-convolution forward      d = k - P, reflect padding                 (Conv2d(cin, cin, k, 1, k//2, reflect))
//   mode 1  its data gradient, EXTENDED domain    position Y = y + P <- g[Y - k], zeros      (folded by the consumer)
//   mode 2  synthesis pre-convolution forward     d = P - k, zeros                           (ConvTranspose2d(cin, cin, k, 1, k//2))
//   mode 3  its data gradient                     d = k - P, zeros
int stride1_corr(const void *in16, int n, int ih, int iw, int ck, const void *packed, int ks, int mode, float *out32,
                 void *out16, int cn, const float *bias, int act, hipStream_t st) {
    if (bad_kernel_size(ks)) return kernel_size_error(ks);
    if (mode < 0 || mode > 3) return fail(CAE_ERR_ARG, "bad mode %d", mode);
    const int P = ks / 2, grow = mode == 1 ? 2 * P : 0;
    GGArgs a = gg_args(in16, n, ih, iw, ck, packed, out32, out16, cn, ih + grow, iw + grow, bias, 1, 1, act);
    a.reflect = mode == 0;
    return mode == 1 ? window_corr(a, ks, 0, -1, st) : mode == 2 ? window_corr(a, ks, P, -1, st) : window_corr(a, ks, -P, 1, st);
}

int pointwise_impl(const void *x16, int n, int h, int w, int ck, const void *packed, float *out32, void *out16, int cn,
                   const float *bias, int act, int acc, hipStream_t st) {
    GGArgs a = gg_args(x16, n, h, w, ck, packed, out32, out16, cn, h, w, bias, 1, 1, act);
    a.acc = acc;
    return window_corr(a, 1, 0, 1, st);
}

// ---- GDN ----
template <int MODE>
int launch_gdn_a(const GdnArgs &a, hipStream_t st) {
    return for_tiles<MAX_CT>(a.C / 32, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        constexpr int LDS = CT * 32 * (CT * 32 + 4) * 4 + (CT <= 4 ? 2 * 32768 : 0);  // M (+ the A double buffer)
        const long tiles = (a.pixels + 255) / 256;
        const unsigned grid = (unsigned)std::min<long>(tiles, 2 * TRAIN_CUS);
        return launch(gdn_gemm_a_kernel<CT, MODE>, dim3(grid), dim3(256), LDS, st, a);
    });
}

template <int CT>
int launch_gdn_b_t(const float *gn, const float *z, long pixels, float *gg, float *gb, hipStream_t st) {
    const unsigned grid = (unsigned)std::min<long>(std::max<long>(pixels / 256, 1), TRAIN_CUS);
    return launch(gdn_gemm_b_kernel<CT>, dim3(grid), dim3(CT * 64), 0, st, gn, z, pixels, gg, gb);
}

constexpr int FUSED_GDN_MAX_CT = 4;  // gdn_fwd_fused_kernel / gdn_bwd_fused_kernel: Gamma and the tile sets fill the LDS above
int fused_gdn_too_wide(int cp) {
    return fail(CAE_ERR_UNSUPPORTED, "fused GDN kernels are built for at most 128 channels, got %d", cp);
}

int launch_gdn_fused(const GdnFusedArgs &a, int cp, bool backward, hipStream_t st) {
    if (cp < 32 || cp > 32 * FUSED_GDN_MAX_CT) return fused_gdn_too_wide(cp);
    return for_tiles<FUSED_GDN_MAX_CT>(cp / 32, [&](auto ct) {
        constexpr int CT = decltype(ct)::value, C = CT * 32;
        constexpr int LDS_F = 2 * 32 * C * 4 + 32 * (C * 2 + 16);  // (Gamma in registers)
        constexpr int LDS_B = C * (C + 4) * 4 + 4 * 32 * C * 4 + 32 * (C * 2 + 16);
        const long tiles = (a.pixels + 31) / 32;
        // persistent blocks walk the tiles: one per CU (backward: Gamma + two tile sets fill the LDS), two per CU (forward)
        const unsigned grid = (unsigned)std::min<long>(tiles, backward ? TRAIN_CUS : 2 * TRAIN_CUS);
        if (!backward) return launch(gdn_fwd_fused_kernel<CT>, dim3(grid), dim3(CT * 64), LDS_F, st, a);
        return launch(gdn_bwd_fused_kernel<CT>, dim3(grid), dim3(CT * 64), LDS_B, st, a);
    });
}

// reflect fold of an extended-domain gradient in place (touches the border pixels only); nothing to do without padding
int fold_in_place(float *gext32, int n, int h, int w, int pad, int cp, hipStream_t st) {
    if (pad <= 0) return CAE_OK;
    return launch(fold_inplace_kernel, dim3((unsigned)(n * (2 * pad + 1))), dim3(256), 0, st, gext32, h, w, pad, cp);
}

// the GDN parameter gradients are accumulated by atomics
int zero_gdn_grads(float *ggamma, float *gbeta, int cp, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(ggamma, 0, (size_t)cp * cp * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(gbeta, 0, (size_t)cp * sizeof(float), st));
    return CAE_OK;
}

// ---- weight gradient ----
// gW[tap] of the k x k window d = k - P over positions S apart (tiles of 8 x 16 positions); k = 1: the pointwise product
int wgrad_impl(const void *xbig16, int n, int h, int w, int ca, const void *ysmall16, int oh, int ow, int cb, int ks,
               int reflect, int S, float *gw32, void *stream) {
    if (!xbig16 || !ysmall16 || !gw32) return fail(CAE_ERR_ARG, "NULL argument");
    if (ks != 1 && bad_kernel_size(ks)) return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (1, 3 or 5)", ks);
    if (bad_channels(ca) || bad_channels(cb)) return fail(CAE_ERR_ARG, "channel counts must be multiples of 32, at most 192");
    hipStream_t st = (hipStream_t)stream;
    WGArgs a{};
    a.S = S;
    a.x = xbig16;
    a.y = ysmall16;
    a.gw = gw32;
    a.zero = zero_page();
    if (!a.zero) return fail(CAE_ERR_NOMEM, "zero page");
    a.N = n;
    a.H = h;
    a.W = w;
    a.Ca = ca;
    a.OH = oh;
    a.OW = ow;
    a.Cb = cb;
    a.reflect = reflect;
    a.kk = ks * ks;
    TapList t;
    add_taps(t, ks, -(ks / 2), -(ks / 2), 1, 1);
    std::copy(t.dy, t.dy + MAX_TAPS, a.dy);
    std::copy(t.dx, t.dx + MAX_TAPS, a.dx);
    set_halo(a, t, S, WG_TILE_ROWS, WG_TILE_COLS);
    a.m_ypp = recip32(cb / 8);
    a.tiles_x = ceil_div(ow, WG_TILE_COLS);
    a.tiles_y = ceil_div(oh, WG_TILE_ROWS);
    a.total_tiles = n * a.tiles_x * a.tiles_y;
    HIP_TRY(hipMemsetAsync(gw32, 0, (size_t)a.kk * ca * cb * sizeof(float), st));
    // staging buffer: the X halo of a 32-channel a-tile + a tile's positions of Y, 16-byte pieces, 64 per instruction
    const int x_instr = halo_instr(4, a.HR, a.HC), y_instr = (WG_TILE_ROWS * WG_TILE_COLS * (cb / 8) + 63) / 64;
    const size_t lds = (size_t)(x_instr + y_instr) * 1024;
    const int a_tiles = ca / 32, tap_groups = (a.kk + 8) / 9;
    // wgrad8_kernel: 8 waves, double-buffered samples; needs two staging buffers in the LDS and Cb <= 128
    // (the 192-channel layers as two launches of 96 b channels measured slower than wgrad_kernel<2>: r03_experiments.md)
    // (at least the 80 KiB in which the position groups merge their partial sums at the end)
    const size_t lds8 = std::max<size_t>(2 * lds, 4 * 5 * 16 * 64 * sizeof(float));
    if (cb <= WG8_MAX_CB && x_instr <= WG8_X_INSTR && lds8 <= LDS_BUDGET) {
        const int tpi = a.tiles_x * a.tiles_y;
        // sample lanes: about ONE block per CU, and at least four samples per block -- every block ends with an atomic flush
        // of its 9 x 32 x Cb partial sums, and that flush, not the contraction, set the time with more blocks
        // (128 -> 128, 128^2 / 64^2 inputs; batch 128: 512 blocks 0.50 / 0.18 ms, 256 blocks 0.46 / 0.14 ms;
        //  batch 16: 512 blocks 0.15 / 0.13 ms, 256 / 128 blocks 0.105 / 0.053 ms)
        const int base = std::max(1, tpi * a_tiles * tap_groups);
        const int step = std::max(1, std::min(std::max(1, n / 4), TRAIN_CUS / base));
        a.Cbs = cb;  // (cb0 = 0: all b channels in one launch)
        return launch(wgrad8_kernel, dim3(tpi * step, a_tiles, tap_groups), dim3(512), lds8, st, a, tpi, step);
    }
    // (about one block per CU here too: 256 blocks 13.06 - 13.11 ms per 128 x 256^2 step, 512: 13.18, 128: 13.15 - 13.18, 64: 13.45 - 13.5)
    const int ksplit = std::max(1, std::min(a.total_tiles, TRAIN_CUS / (a_tiles * tap_groups)));
    const dim3 grid(ksplit, a_tiles, tap_groups);  // (wgrad_kernel<NB>: NB b-tiles per wave)
    return cb / 32 <= 4 ? launch(wgrad_kernel<1>, grid, dim3(256), lds, st, a)
                        : launch(wgrad_kernel<2>, grid, dim3(256), lds, st, a);
}

// the strided layers' forwards; `bad` is the entry point's text for a bad shape
int conv_forward(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16, int cout_p,
                 const float *bias, int act, const char *bad, void *stream) {
    if (!x16 || !packed || (!z32 && !z16)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 2 || w < 2 || act < 0 || act > 2) return fail(CAE_ERR_ARG, "%s", bad);
    return strided_corr(x16, n, h, w, cin_p, packed, ks, 1, z32, z16, cout_p, (h + 1) / 2, (w + 1) / 2, bias, act,
                        (hipStream_t)stream);
}

int deconv_forward(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                   int cout_p, const float *bias, int act, const char *bad, void *stream) {
    if (!x16 || !packed || (!z32 && !z16)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || act < 0 || act > 2) return fail(CAE_ERR_ARG, "%s", bad);
    return strided_corr_t(x16, n, h, w, cin_p, packed, ks, ks / 2, z32, z16, cout_p, 2 * h, 2 * w, bias, act,
                          (hipStream_t)stream);
}

}  // namespace

extern "C" {

int cae_t_set_samples_per_block(int npb) {
    if (npb < 0) return fail(CAE_ERR_ARG, "samples per block must be 0 (automatic) or positive, got %d", npb);
    g_samples_per_block.store(npb, std::memory_order_relaxed);
    return CAE_OK;
}

size_t cae_t_packed_bytes(int contract_channels, int out_channels, int kernel_size) {
    const size_t q = (contract_channels + 31) / 32, nt = (out_channels + 31) / 32;
    return q * kernel_size * kernel_size * nt * 2 * 512 * 2;
}

int cae_t_pack_weights(const float *w, int dim0, int dim1, int ks, int contract_dim, void *packed, void *stream) {
    if (!w || !packed) return fail(CAE_ERR_ARG, "NULL argument");
    if (dim0 < 1 || dim1 < 1 || (contract_dim != 0 && contract_dim != 1)) return fail(CAE_ERR_ARG, "bad weight shape");
    const int kk = ks * ks;
    const int Kc = contract_dim == 0 ? dim0 : dim1, Nc = contract_dim == 0 ? dim1 : dim0;
    const long s0 = (long)dim1 * kk, s1 = kk;  // element strides of dim0 / dim1
    const long sk = contract_dim == 0 ? s0 : s1, sn = contract_dim == 0 ? s1 : s0;
    const int kchunks = (Kc + 31) / 32, NT = (Nc + 31) / 32;
    const size_t total = (size_t)kchunks * kk * NT * 1024;
    return launch_ew(pack_weights_kernel, total, stream, w, (__bf16 *)packed, Kc, Nc, kk, sk, sn, kchunks, NT);
}

int cae_t_from_nchw(const float *x, int n, int c, int h, int w, int cp, void *out16, float *out32, void *stream) {
    if (!x || (!out16 && !out32)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || h < 1 || w < 1 || cp < c || cp % 32) return fail(CAE_ERR_ARG, "bad shape");
    return launch_ew(nchw_to_t_kernel, (size_t)n * h * w * cp, stream, x, (__bf16 *)out16, out32, n, c, h, w, cp);
}

int cae_t_to_nchw(const float *t32, int n, int c, int h, int w, int cp, float *out, void *stream) {
    if (!t32 || !out) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || h < 1 || w < 1 || cp < c || cp % 32) return fail(CAE_ERR_ARG, "bad shape");
    return launch_ew(t_to_nchw_kernel, (size_t)n * c * h * w, stream, t32, out, n, c, h, w, cp);
}

int cae_t_conv_forward(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                       int cout_p, const float *bias, void *stream) {
    return conv_forward(x16, n, h, w, cin_p, packed, ks, z32, z16, cout_p, bias, 0, "bad shape", stream);
}

int cae_t_conv_forward_act(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                           int cout_p, const float *bias, int act, void *stream) {
    return conv_forward(x16, n, h, w, cin_p, packed, ks, z32, z16, cout_p, bias, act, "bad shape or activation", stream);
}

int cae_t_deconv_forward(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                         int cout_p, const float *bias, void *stream) {
    return deconv_forward(x16, n, h, w, cin_p, packed, ks, z32, z16, cout_p, bias, 0, "bad shape", stream);
}

int cae_t_deconv_forward_act(const void *x16, int n, int h, int w, int cin_p, const void *packed, int ks, float *z32, void *z16,
                             int cout_p, const float *bias, int act, void *stream) {
    return deconv_forward(x16, n, h, w, cin_p, packed, ks, z32, z16, cout_p, bias, act, "bad shape or activation", stream);
}

int cae_t_corr_s1(const void *x16, int n, int h, int w, int ck, const void *packed, int ks, int mode, float *out32, void *out16,
                  int cn, const float *bias, int act, void *stream) {
    if (!x16 || !packed || (!out32 && !out16)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || act < 0 || act > 2) return fail(CAE_ERR_ARG, "bad shape or activation");
    return stride1_corr(x16, n, h, w, ck, packed, ks, mode, out32, out16, cn, bias, act, (hipStream_t)stream);
}

int cae_t_pointwise(const void *x16, int n, int h, int w, int ck, const void *packed, float *out32, void *out16, int cn,
                    const float *bias, int act, void *stream) {
    if (!x16 || !packed || (!out32 && !out16)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || act < 0 || act > 2) return fail(CAE_ERR_ARG, "bad shape or activation");
    return pointwise_impl(x16, n, h, w, ck, packed, out32, out16, cn, bias, act, 0, (hipStream_t)stream);
}

int cae_t_pointwise_acc(const void *x16, int n, int h, int w, int ck, const void *packed, float *out32, int cn, void *stream) {
    if (!x16 || !packed || !out32) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad shape");
    return pointwise_impl(x16, n, h, w, ck, packed, out32, nullptr, cn, nullptr, 0, 1, (hipStream_t)stream);
}

int cae_t_col2im_s1r(const float *u32, const float *bias, int n, int c, int h, int w, int ks, int kp, float *out_nchw,
                     void *stream) {
    if (!u32 || !out_nchw) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || c > 3 || bad_kernel_size(ks) || kp % 32 || kp < ks * ks * c || kp > 96)
        return fail(CAE_ERR_ARG, "bad shape (1 to 3 channels, kernel_size 3 or 5, kp = pad32(k * k * c) <= 96)");
    if (h <= ks / 2 || w <= ks / 2) return fail(CAE_ERR_ARG, "image %d x %d too small for reflect padding %d", h, w, ks / 2);
    return launch_ew(col2im_s1r_kernel, (size_t)n * h * w, stream, u32, bias, out_nchw, n, c, h, w, ks, kp);
}

int cae_t_im2col_s1r(const float *g_nchw, int n, int c, int h, int w, int ks, int kp, void *out16, void *stream) {
    if (!g_nchw || !out16) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || c > 3 || bad_kernel_size(ks) || kp % 32 || kp < ks * ks * c || kp > 96)
        return fail(CAE_ERR_ARG, "bad shape (1 to 3 channels, kernel_size 3 or 5, kp = pad32(k * k * c) <= 96)");
    if (h <= ks / 2 || w <= ks / 2) return fail(CAE_ERR_ARG, "image %d x %d too small for reflect padding %d", h, w, ks / 2);
    return launch_ew(im2col_s1r_kernel, (size_t)n * h * w * (kp / 8), stream, g_nchw, (__bf16 *)out16, n, c, h, w, ks, kp);
}

int cae_t_fold_acc(const float *gext32, int n, int h, int w, int pad, int cp, float *out32, void *stream) {
    if (!gext32 || !out32) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h <= pad || w <= pad || pad < 0 || cp % 32) return fail(CAE_ERR_ARG, "bad shape");
    return launch_ew(fold_acc_kernel, (size_t)n * h * w * cp, stream, FoldSrc{gext32, h, w, pad}, out32, n, cp);
}

int cae_t_pyramid_down(const float *x_nchw, int n, int c, int h, int w, float *out_nchw, void *stream) {
    if (!x_nchw || !out_nchw) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || h < 2 || w < 2) return fail(CAE_ERR_ARG, "bad shape (the pyramid step needs h, w >= 2)");
    const int oh = h / 2, ow = w / 2;
    return launch_ew(pyramid_down_kernel, (size_t)n * c * oh * ow, stream, x_nchw, out_nchw, n * c, h, w, oh, ow);
}

int cae_t_im2col_s2(const float *x_nchw, int n, int c, int h, int w, int oh, int ow, int ks, int reflect, void *out16,
                    void *stream) {
    if (!x_nchw || !out16) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || bad_kernel_size(ks) || ks * ks * c > 32)
        return fail(CAE_ERR_ARG, "bad shape (kernel_size^2 * channels must fit 32)");
    return launch_ew(im2col_s2_kernel, (size_t)n * oh * ow * 4, stream, x_nchw, (__bf16 *)out16, n, c, h, w, oh, ow, ks,
                     reflect);
}

int cae_t_col2im_s2(const float *u32, const float *bias, int n, int c, int h, int w, int ks, float *out_nchw, void *stream) {
    if (!u32 || !out_nchw) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || h < 1 || w < 1 || bad_kernel_size(ks) || ks * ks * c > 32)
        return fail(CAE_ERR_ARG, "bad shape (kernel_size^2 * channels must fit 32)");
    return launch_ew(col2im_s2_kernel, (size_t)n * 4 * h * w, stream, u32, bias, out_nchw, n, c, h, w, ks);
}

int cae_t_act_backward(const void *g16, float *gext32, int pad, const void *y16, int n, int h, int w, int cp, int act,
                       void *out16, void *stream) {
    if ((!g16 && !gext32) || !y16 || !out16) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || pad < 0 || cp % 32 || act < 1 || act > 2) return fail(CAE_ERR_ARG, "bad shape or activation");
    hipStream_t st = (hipStream_t)stream;
    if (!g16) CAE_TRY(fold_in_place(gext32, n, h, w, pad, cp, st));
    return launch_ew(act_bwd_kernel, (size_t)n * h * w * cp, st, (const __bf16 *)g16, FoldSrc{gext32, h, w, g16 ? 0 : pad},
                     (const __bf16 *)y16, act == 1 ? 0.01f : 0.0f, (__bf16 *)out16, n, h, w, cp);
}

int cae_t_conv_dgrad_ext(const void *gz16, int n, int oh, int ow, int cout_p, const void *packed, int ks, int h, int w,
                         float *gext32, int cin_p, void *stream) {
    if (!gz16 || !packed || !gext32) return fail(CAE_ERR_ARG, "NULL argument");
    if (oh != (h + 1) / 2 || ow != (w + 1) / 2) return fail(CAE_ERR_ARG, "gradient shape does not match the input shape");
    const int P = ks / 2, eh = h + 2 * P, ew = w + 2 * P;
    // (every position of the extended domain belongs to exactly one of the four output parities and each of them has at
    //  least one tap for k >= 2, so all of gext32 is written: positions beyond 2 oh + k - 2 (odd input sizes) read
    //  nothing but the zero page and come out as 0 -- no memset of the ~1 GB tensor)
    return strided_corr_t(gz16, n, oh, ow, cout_p, packed, ks, 0, gext32, nullptr, cin_p, eh, ew, nullptr, 0, (hipStream_t)stream);
}

int cae_t_deconv_dgrad(const void *gz16, int n, int h, int w, int cout_p, const void *packed, int ks, float *gx32, void *gx16,
                       int cin_p, void *stream) {
    if (!gz16 || !packed || (!gx32 && !gx16)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad shape");
    return strided_corr(gz16, n, 2 * h, 2 * w, cout_p, packed, ks, 0, gx32, gx16, cin_p, h, w, nullptr, 0, (hipStream_t)stream);
}

int cae_t_wgrad(const void *xbig16, int n, int h, int w, int ca, const void *ysmall16, int oh, int ow, int cb, int ks,
                int reflect, float *gw32, void *stream) {
    if (n < 1 || oh < 1 || ow < 1 || 2 * oh < h || 2 * ow < w) return fail(CAE_ERR_ARG, "bad shape");
    return wgrad_impl(xbig16, n, h, w, ca, ysmall16, oh, ow, cb, ks, reflect, 2, gw32, stream);
}

int cae_t_wgrad_s1(const void *x16, int n, int h, int w, int ca, const void *y16, int cb, int ks, int reflect, float *gw32,
                   void *stream) {
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad shape");
    return wgrad_impl(x16, n, h, w, ca, y16, h, w, cb, ks, reflect, 1, gw32, stream);
}

int cae_t_wgrad_pointwise(const void *x16, const void *y16, int n, int h, int w, int ca, int cb, float *gw32, void *stream) {
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad shape");
    return wgrad_impl(x16, n, h, w, ca, y16, h, w, cb, 1, 0, 1, gw32, stream);
}

int cae_t_gdn_forward(const float *z32, long pixels, int cp, const float *beta, const float *gamma, int inverse, float *y32,
                      void *y16, void *stream) {
    if (!z32 || !beta || !gamma || (!y32 && !y16)) return fail(CAE_ERR_ARG, "NULL argument");
    if (pixels < 1 || bad_channels(cp)) return fail(CAE_ERR_ARG, "bad shape");
    GdnArgs a{};
    a.a = z32;
    a.mat = gamma;
    a.beta = beta;
    a.z = z32;
    a.o32a = y32;
    a.o16 = y16;
    a.pixels = pixels;
    a.C = cp;
    a.inverse = inverse;
    return launch_gdn_a<0>(a, (hipStream_t)stream);
}

int cae_t_gdn_backward(const float *z32, const float *gext32, int n, int h, int w, int pad, int cp, const float *beta,
                       const float *gamma, const float *gamma_t, int inverse, float *gn_ws32, float *gzd_ws32, float *gz32,
                       void *gz16, float *ggamma, float *gbeta, void *stream) {
    if (!z32 || !gext32 || !beta || !gamma || !gamma_t || !gn_ws32 || !gzd_ws32 || (!gz32 && !gz16) || !ggamma || !gbeta)
        return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || pad < 0 || bad_channels(cp)) return fail(CAE_ERR_ARG, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    const long pixels = (long)n * h * w;
    if (pixels >= (1l << 31)) return fail(CAE_ERR_ARG, "more than 2^31 pixels per call");
    GdnArgs a{};
    a.a = z32;
    a.mat = gamma;
    a.beta = beta;
    a.z = z32;
    a.gy = FoldSrc{gext32, h, w, pad};
    a.img_h = h;
    a.img_w = w;
    a.o32a = gn_ws32;
    a.o32b = gzd_ws32;
    a.pixels = pixels;
    a.C = cp;
    a.inverse = inverse;
    CAE_TRY(launch_gdn_a<1>(a, st));
    GdnArgs b{};
    b.a = gn_ws32;
    b.mat = gamma_t;
    b.z = z32;
    b.o32a = gz32;
    b.o32b = gzd_ws32;
    b.o16 = gz16;
    b.pixels = pixels;
    b.C = cp;
    b.inverse = inverse;
    CAE_TRY(launch_gdn_a<2>(b, st));
    CAE_TRY(zero_gdn_grads(ggamma, gbeta, cp, st));
    return for_tiles<MAX_CT>(cp / 32, [&](auto ct) {
        return launch_gdn_b_t<decltype(ct)::value>(gn_ws32, z32, pixels, ggamma, gbeta, st);
    });
}

size_t cae_t_gdn_saved_elems(long pixels, int cp) {
    if (pixels < 1 || cp < 32 || cp > 32 * FUSED_GDN_MAX_CT || cp % 32) return 0;
    return (size_t)((pixels + 63) / 64) * 64 * (size_t)cp;
}

int cae_t_gdn_forward_save(const float *z32, long pixels, int cp, const float *beta, const float *gamma, int inverse,
                           void *y16, float *f_saved, void *stream) {
    if (!z32 || !beta || !gamma || !y16 || !f_saved) return fail(CAE_ERR_ARG, "NULL argument");
    if (pixels < 1 || pixels >= (1l << 31) || cp % 32) return fail(CAE_ERR_ARG, "bad shape");
    GdnFusedArgs a{};
    a.z = z32;
    a.gamma = gamma;
    a.beta = beta;
    a.f = f_saved;
    a.y16 = y16;
    a.pixels = pixels;
    a.inverse = inverse;
    return launch_gdn_fused(a, cp, false, (hipStream_t)stream);
}

int cae_t_gdn_backward_fused(const float *z32, const float *f_saved, float *gext32, int n, int h, int w, int pad, int cp,
                             const float *gamma, int inverse, void *gz16, float *ggamma, float *gbeta, void *stream) {
    if (!z32 || !f_saved || !gext32 || !gamma || !gz16 || !ggamma || !gbeta) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || pad < 0 || cp % 32) return fail(CAE_ERR_ARG, "bad shape");
    const long pixels = (long)n * h * w;
    if (pixels >= (1l << 31)) return fail(CAE_ERR_ARG, "more than 2^31 pixels per call");
    if (cp > 32 * FUSED_GDN_MAX_CT) return fused_gdn_too_wide(cp);
    hipStream_t st = (hipStream_t)stream;
    CAE_TRY(zero_gdn_grads(ggamma, gbeta, cp, st));
    CAE_TRY(fold_in_place(gext32, n, h, w, pad, cp, st));
    GdnFusedArgs a{};
    a.z = z32;
    a.gamma = gamma;
    a.f = const_cast<float *>(f_saved);
    a.gy = FoldSrc{gext32, h, w, pad};
    a.img_h = h;
    a.img_w = w;
    a.gz16 = gz16;
    a.ggamma = ggamma;
    a.gbeta = gbeta;
    a.pixels = pixels;
    a.inverse = inverse;
    return launch_gdn_fused(a, cp, true, st);
}

int cae_t_fold_to_bf16(const float *gext32, int n, int h, int w, int pad, int cp, void *out16, void *stream) {
    if (!gext32 || !out16) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || pad < 0 || cp % 32) return fail(CAE_ERR_ARG, "bad shape");
    return launch_ew(fold_to_bf16_kernel, (size_t)n * h * w * cp, stream, FoldSrc{gext32, h, w, pad}, (__bf16 *)out16, n, cp);
}

int cae_t_bn_moments(const float *a, const float *b, int n, int c, long hw, double *s1, double *s2, void *stream) {
    if (!a || !b || !s1 || !s2) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || c > 65535 || hw < 1) return fail(CAE_ERR_ARG, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(s1, 0, (size_t)c * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(s2, 0, (size_t)c * sizeof(double), st));
    const long total = (long)n * hw;
    const unsigned splits = (unsigned)std::min<long>(std::max<long>(total / 4096, 1), std::max<long>(2048 / c, 1));
    return launch(bn_moments_kernel, dim3((unsigned)c, splits), dim3(256), 0, st, a, b, n, c, hw, s1, s2);
}

int cae_t_bn_affine(const float *a, const float *b, int n, int c, long hw, const float *A, const float *B, const float *C,
                    float *out, void *stream) {
    if (!a || !A || !C || !out || (b && !B)) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || c < 1 || hw < 1) return fail(CAE_ERR_ARG, "bad shape");
    const size_t total = (size_t)n * c * hw;
    return launch_ew(bn_affine_kernel, total, stream, a, b, c, hw, total, A, B, C, out);
}

int cae_t_colsum(const void *g16, long pixels, int cp, float *out, void *stream) {
    if (!g16 || !out) return fail(CAE_ERR_ARG, "NULL argument");
    if (pixels < 1 || cp % 32 || cp > 256) return fail(CAE_ERR_ARG, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)cp * sizeof(float), st));
    const int threads = (256 / cp) * cp;
    const long rows = 256 / cp;
    const unsigned grid = (unsigned)std::min<long>(std::max<long>((pixels + rows - 1) / rows, 1), 1024);
    return launch(colsum_bf16_kernel, dim3(grid), dim3(threads), 0, st, (const __bf16 *)g16, pixels, cp, out);
}

}  // extern "C"
