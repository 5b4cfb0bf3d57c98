// (generated split of the launcher code: one translation unit per kernel family so hipcc
//  compiles them in parallel; see cae_launch.hpp)
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"
#include "cae_kernels_f16.hpp"
namespace cae {
constexpr int LDS_LIMIT = 160 * 1024;

// LDS of conv_s2_f16_kernel<KS, CT, GDN, S>: two stage buffers, each the weights of one kernel row + the halo (16 rows
// of `wh` columns), or a stage of gamma when that is larger
constexpr int conv_f16_lds(int ks, int ct, bool gdn, int wh) {
    const int halo_instr = (4 * 16 * wh + 63) / 64;
    const int conv_stage = ks * ct * 2 * 1024 + halo_instr * 1024;
    const int g_bytes = gdn ? ct * 4096 : 0;
    return 2 * (conv_stage > g_bytes ? conv_stage : g_bytes);
}
constexpr int conv_f16_halo_width(int ks, int stride) { return stride * 16 + ks - stride; }

// (k = 5 with 192 output channels needs 192 KiB: such a layer runs on the fp32 kernel instead)
bool conv_f16_fits(int ks, int ct, bool gdn) {
    if (gdn && ct > 4) gdn = false;  // wider than 128 channels: convolution without the epilogue + gdn_f16_kernel
    return conv_f16_lds(ks, ct, gdn, conv_f16_halo_width(ks, 2)) <= LDS_LIMIT;
}

// conv_s2_f16_kernel: tiles of 16 x 16 output pixels, 16-channel contraction chunks
static LayerArgs conv_f16_facts(const LayerArgs &a, int cin) {
    return with_launch_facts(a, a.OW, a.OH, 16, 16, (cin + 15) / 16);
}

template <int KS, int CT, bool GDN>
static int launch_conv_f16_t(int cin, const LayerArgs &args, hipStream_t st) {
    constexpr int NW = CONV_F16_NW;
    constexpr int LDS = conv_f16_lds(KS, CT, GDN, conv_f16_halo_width(KS, 2));
    if constexpr (LDS > LDS_LIMIT) {
        return fail(CAE_ERR_UNSUPPORTED, "f16x3: this kernel_size/channel combination exceeds the LDS; use fp32");
    } else {
        auto kern = conv_s2_f16_kernel<KS, CT, GDN>;
        CAE_TRY(ensure_lds((const void *)kern, LDS));
        const LayerArgs a = conv_f16_facts(args, cin);
        const unsigned grid = (unsigned)((size_t)a.N * a.tiles_x * a.tiles_y);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), LDS, st, a);
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
}

#define DISPATCH_F16(FN, KS_)                                                               \
    switch (ct) {                                                                          \
        case 1: return gdn ? FN<KS_, 1, true>(cin, a, st) : FN<KS_, 1, false>(cin, a, st); \
        case 2: return gdn ? FN<KS_, 2, true>(cin, a, st) : FN<KS_, 2, false>(cin, a, st); \
        case 4: return gdn ? FN<KS_, 4, true>(cin, a, st) : FN<KS_, 4, false>(cin, a, st); \
        case 6: { /* wider than 128 channels: the normalisation runs as a kernel of its own */ \
            const int rc6 = FN<KS_, 6, false>(cin, a, st);                                 \
            return rc6 || !gdn ? rc6 : launch_gdn_f16(6, false, a, st);                    \
        }                                                                                  \
        default: return fail(CAE_ERR_UNSUPPORTED, "unsupported channel tiles %d", ct);      \
    }

// stride-1 stage of a LeakyReLU / ReLU unit or of a residual unit.  Epilogue: GDN (analysis) / IGDN (synthesis) or the
// activation a.act, then -- up to 128 channels -- + a.res and a.post_act.  SYN: C8SP rows; ZP: zero padding (the synthesis
// units' transposed convolutions) instead of reflection (analysis units, and the colour layers of the synthesis track).
template <int KS, int CT, bool GDN, bool SYN, bool ZP>
static int launch_conv_s1_f16_t(int cin, const LayerArgs &args, hipStream_t st) {
    constexpr int NW = CONV_F16_NW;
    constexpr int LDS = conv_f16_lds(KS, CT, GDN, conv_f16_halo_width(KS, 1));
    if constexpr (LDS > LDS_LIMIT) {
        return fail(CAE_ERR_UNSUPPORTED, "f16x3: this kernel_size/channel combination exceeds the LDS; use fp32");
    } else {
        auto kern = conv_s2_f16_kernel<KS, CT, GDN, 1, SYN, ZP, (CT <= 4)>;
        CAE_TRY(ensure_lds((const void *)kern, LDS));
        const LayerArgs a = conv_f16_facts(args, cin);
        const unsigned grid = (unsigned)((size_t)a.N * a.tiles_x * a.tiles_y);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), LDS, st, a);
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
}

int launch_conv_s1_f16(int ks, int ct, bool synthesis, bool gdn, int cin, const LayerArgs &a, hipStream_t st) {
    if ((gdn || a.res || a.post_act) && ct > 4)
        return fail(CAE_ERR_UNSUPPORTED, "f16x3: GDN / residual stages wider than 128 channels run on the fp32 path");
#define S1_SIDE(KS_, CT_, GDN_) \
    return synthesis ? launch_conv_s1_f16_t<KS_, CT_, GDN_, true, true>(cin, a, st) \
                     : launch_conv_s1_f16_t<KS_, CT_, GDN_, false, false>(cin, a, st)
#define S1_CASE(KS_)                                                                   \
    switch (ct) {                                                                      \
        case 1: if (gdn) { S1_SIDE(KS_, 1, true); } else { S1_SIDE(KS_, 1, false); }   \
        case 2: if (gdn) { S1_SIDE(KS_, 2, true); } else { S1_SIDE(KS_, 2, false); }   \
        case 4: if (gdn) { S1_SIDE(KS_, 4, true); } else { S1_SIDE(KS_, 4, false); }   \
        case 6: S1_SIDE(KS_, 6, false);                                                \
        default: return fail(CAE_ERR_UNSUPPORTED, "unsupported channel tiles %d", ct);  \
    }
    if (ks == 3) { S1_CASE(3) }
    if (ks == 5) { S1_CASE(5) }
#undef S1_CASE
#undef S1_SIDE
    return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks);
}

// multiscale colour layer (_autoencoders.py:417-436): reflect convolution of a synthesis level (C8SP rows) to the image
// channels, NCHW fp32 out
int launch_color_f16(int ks, int cin, const LayerArgs &a, hipStream_t st) {
    if (ks == 3) return launch_conv_s1_f16_t<3, 1, false, true, false>(cin, a, st);
    if (ks == 5) return launch_conv_s1_f16_t<5, 1, false, true, false>(cin, a, st);
    return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks);
}

int launch_conv_f16(int ks, int ct, bool gdn, int cin, const LayerArgs &a, hipStream_t st) {
    if (ks == 3) { DISPATCH_F16(launch_conv_f16_t, 3) }
    if (ks == 5) { DISPATCH_F16(launch_conv_f16_t, 5) }
    return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks);
}

}  // namespace cae
