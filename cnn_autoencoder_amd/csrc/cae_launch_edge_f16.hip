// (generated split of the launcher code: one translation unit per kernel family so hipcc
//  compiles them in parallel; see cae_launch.hpp)
#include <algorithm>

#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_launch.hpp"
#include "cae_kernels_f16.hpp"
namespace cae {
// Launch shape of the three persistent kernels of this file: what the kernel's loop counts (`tiles`), the grid on the
// current device (`blocks`: one block per CU at the most, a block takes tiles b, b + blocks, ...) and the launch facts
// of the kernel's tile.  The launchers and cae_persistent_launch (the tests) read it here and nowhere else.
struct PersistentShape {
    size_t tiles;
    unsigned blocks;
    LayerArgs args;  // the caller's arguments with tiles_x, tiles_y and cci filled in (gdn_f16_kernel: as given)
};

static int persistent_shape(const LayerArgs &b, size_t tiles, size_t tiles_per_block, PersistentShape &s) {
    int n_cu = 0;
    CAE_TRY(device_cus(n_cu));
    if (tiles > 0x7fffffff) return fail(CAE_ERR_ARG, "batch too large");
    s.tiles = tiles;
    s.blocks = (unsigned)std::min<size_t>((tiles + tiles_per_block - 1) / tiles_per_block, (size_t)std::max(n_cu, 1));
    s.args = b;
    return CAE_OK;
}

// conv_first_f16_kernel: tiles of TX x TY output pixels (a.N, a.OH, a.OW), the same for every instantiation
using FirstTile = FirstGeomF16<3, 1, false>;
static int first_f16_shape(const LayerArgs &a, int cin, PersistentShape &s) {
    const LayerArgs b = with_launch_facts(a, a.OW, a.OH, FirstTile::TX, FirstTile::TY, (cin + 7) / 8);
    return persistent_shape(b, (size_t)b.N * b.tiles_x * b.tiles_y, 1, s);
}

// gdn_f16_kernel: every wave of a 4-wave block takes 32-pixel groups of the split rows (a.N, a.OH, a.OW)
template <bool INVERSE>
static int gdn_f16_shape(const LayerArgs &a, PersistentShape &s) {
    const size_t groups = c8s_row_bytes<INVERSE>(a.OW) / 1024;
    return persistent_shape(a, (size_t)a.N * a.OH * groups, 4, s);
}

// deconv_last_f16_kernel: tiles of TXC x NW input pixels (a.N, a.H, a.W), 32-channel contraction groups
template <class G>
static int last_f16_shape(const LayerArgs &a, int cin, PersistentShape &s) {
    const LayerArgs b = with_launch_facts(a, a.W, a.H, G::TXC, G::NW, (cin + 31) / 32);
    return persistent_shape(b, (size_t)b.N * b.tiles_x * b.tiles_y, 1, s);
}

template <int KS, int CT, bool GDN>
static int launch_first_f16_t(const LayerArgs &a, const FirstArgs &f, hipStream_t st) {
    using G = FirstGeomF16<KS, CT, GDN>;
    constexpr int LDS = G::LDS_BYTES;
    if constexpr (LDS > 160 * 1024) {
        return fail(CAE_ERR_UNSUPPORTED, "f16x3: first-layer operands exceed the LDS for this shape; use fp32");
    } else {
        auto kern_u8 = conv_first_f16_kernel<KS, CT, GDN, true>;
        auto kern_f32 = conv_first_f16_kernel<KS, CT, GDN, false>;
        static_assert(G::TX == FirstTile::TX && G::TY == FirstTile::TY, "one output tile for every instantiation");
        CAE_TRY(ensure_lds((const void *)kern_u8, LDS));
        CAE_TRY(ensure_lds((const void *)kern_f32, LDS));
        PersistentShape s;  // persistent: one block per CU walks over the tiles
        CAE_TRY(first_f16_shape(a, f.cin, s));
        hipLaunchKernelGGL(f.in_is_u8 ? kern_u8 : kern_f32, dim3(s.blocks), dim3(G::NW * 64), LDS, st, s.args, f);
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
}

int launch_first_f16(int ks, int ct, bool gdn, const LayerArgs &a, const FirstArgs &f, hipStream_t st) {
#define FIRST_F16(KS_)                                                                                       \
    switch (ct) {                                                                                            \
        case 1: return gdn ? launch_first_f16_t<KS_, 1, true>(a, f, st) : launch_first_f16_t<KS_, 1, false>(a, f, st); \
        case 2: return gdn ? launch_first_f16_t<KS_, 2, true>(a, f, st) : launch_first_f16_t<KS_, 2, false>(a, f, st); \
        case 4: return gdn ? launch_first_f16_t<KS_, 4, true>(a, f, st) : launch_first_f16_t<KS_, 4, false>(a, f, st); \
        case 6: {                                                                                            \
            const int rc6 = launch_first_f16_t<KS_, 6, false>(a, f, st);                                     \
            return rc6 || !gdn ? rc6 : launch_gdn_f16(6, false, a, st);                                      \
        }                                                                                                    \
        default: return fail(CAE_ERR_UNSUPPORTED, "unsupported channel tiles %d", ct);                       \
    }
    if (ks == 3) { FIRST_F16(3) }
    if (ks == 5) { FIRST_F16(5) }
    return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks);
}

template <int CT, bool INVERSE>
static int launch_gdn_f16_t(const LayerArgs &a, hipStream_t st) {
    constexpr int LDS = CT * CT * 4096 + CT * 32 * 4;
    static_assert(LDS <= 160 * 1024, "packed gamma must fit the LDS");
    auto kern = gdn_f16_kernel<CT, INVERSE, INVERSE>;  // analysis rows are C8S, synthesis rows C8SP
    CAE_TRY(ensure_lds((const void *)kern, LDS));
    PersistentShape s;  // persistent; wave tiles of 32 pixels
    CAE_TRY((gdn_f16_shape<INVERSE>(a, s)));
    hipLaunchKernelGGL(kern, dim3(s.blocks), dim3(256), LDS, st, s.args);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_gdn_f16(int ct, bool inverse, const LayerArgs &a, hipStream_t st) {
    if (a.outfmt != OUT_C8) return fail(CAE_ERR_UNSUPPORTED, "f16x3: stand-alone GDN needs split rows as output");
    if (ct == 6) return inverse ? launch_gdn_f16_t<6, true>(a, st) : launch_gdn_f16_t<6, false>(a, st);
    return fail(CAE_ERR_UNSUPPORTED, "stand-alone GDN is built for 192-channel layers (channel tiles %d)", ct);
}

// deconv_last_f16_kernel as it is built per kernel size: <3, 8, 3>: 3 x 40 KiB ring + 32 KiB weights (128 channels);
// <5, 4, 2>: 3x3 neighbours, 72 KiB of weights, shallower ring.  Halo ring + all weights resident: a last layer with
// more than 160 input channels does not fit
using LastF16K3 = LastGeomF16<3, 8, 3>;
using LastF16K5 = LastGeomF16<5, 4, 2>;

bool last_f16_fits(int ks, int cin) {
    const int nq = (cin + 31) / 32;
    return (ks == 3 ? LastF16K3::lds_bytes(nq) : LastF16K5::lds_bytes(nq)) <= 160 * 1024;
}

template <int KS, class G>
static int launch_last_f16_t(int cin, const LayerArgs &a, hipStream_t st) {
    constexpr int NW = G::NW, DEPTH = G::DEPTH;
    const int lds = G::lds_bytes((cin + 31) / 32);
    if (lds > 160 * 1024) return fail(CAE_ERR_UNSUPPORTED, "last-layer weights do not fit the LDS");
    auto kern = deconv_last_f16_kernel<KS, NW, DEPTH>;
    CAE_TRY(ensure_lds((const void *)kern, 160 * 1024));
    PersistentShape s;  // persistent
    CAE_TRY(last_f16_shape<G>(a, cin, s));
    hipLaunchKernelGGL(kern, dim3(s.blocks), dim3(NW * 64), lds, st, s.args);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int launch_last_f16(int ks, int cin, const LayerArgs &a, hipStream_t st) {
    if (ks == 3) return launch_last_f16_t<3, LastF16K3>(cin, a, st);
    if (ks == 5) return launch_last_f16_t<5, LastF16K5>(cin, a, st);
    return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", ks);
}

}  // namespace cae

extern "C" int cae_persistent_launch(int kernel, int ks, int n, int h, int w, int64_t *tiles, int *blocks) {
    using namespace cae;
    if (kernel < 0 || kernel > 3 || n < 1 || h < 1 || w < 1 || !tiles || !blocks)
        return fail(CAE_ERR_ARG, "cae_persistent_launch: bad arguments (kernel %d, n %d, h %d, w %d)", kernel, n, h, w);
    if (kernel <= 1 && ks != 3 && ks != 5)
        return fail(CAE_ERR_ARG, "cae_persistent_launch: kernel_size %d not supported (3 or 5)", ks);
    LayerArgs a{};
    a.N = n;
    a.H = a.OH = h;
    a.W = a.OW = w;
    PersistentShape s;
    switch (kernel) {
        case 0: CAE_TRY(first_f16_shape(a, 1, s)); break;
        case 1: CAE_TRY(ks == 3 ? last_f16_shape<LastF16K3>(a, 32, s) : last_f16_shape<LastF16K5>(a, 32, s)); break;
        case 2: CAE_TRY(gdn_f16_shape<false>(a, s)); break;
        default: CAE_TRY(gdn_f16_shape<true>(a, s)); break;
    }
    *tiles = (int64_t)s.tiles;
    *blocks = (int)s.blocks;
    return CAE_OK;
}
