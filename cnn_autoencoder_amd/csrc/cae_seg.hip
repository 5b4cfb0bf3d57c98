// Segmentation head handle (cae_seg_*, include/cae_hip.h): JNet inference on latents and decoder bridges.
#include <climits>
#include <cstring>
#include <mutex>
#include <vector>

#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_kernels_seg.hpp"
#include "cae_launch.hpp"
#include "cae_launch_seg.hpp"
#include "cae_pack.hpp"

namespace cae {

thread_local int64_t g_seg_ticket = 0;  // range ticket of this thread's latest cae_seg_forward

// One convolution of the head with the GroupNorm that follows it (if any)
struct SegLayer {
    int ks = 1, cin_a = 0, cin_b = 0, cout = 0;
    bool up = false;
    int ct = 1, groups = 1, chunks = 1, cp = 8;  // cp: channels of the output's plane grid
    DevBuf wp, bias;
    bool norm = false;  // followed by GroupNorm + ReLU (applied by the consumer)
    DevBuf gamma, beta;  // [cp], zero padded
};

struct Seg {
    cae_seg_config cfg;
    std::vector<SegLayer> st;  // in launch order
    DevBuf proj_gamma[8], proj_beta[8];  // the projection units' _bn1 (on the bridges)
    enum { X0, T1, T2, U, BC, RP, AB, STATS, NWS };
    DevBuf ws[NWS];
    std::mutex mu;
    static constexpr int kFlagSlots = 1024;
    int *flags = nullptr, *flags_dev = nullptr;
    int64_t flag_seq = 0;
    void *last_stream = nullptr;
    bool last_stream_set = false;
    hipEvent_t order_event = nullptr;

    int ensure_ws(int which, size_t bytes) {
        DevBuf &b = ws[which];
        if (b.bytes >= bytes) return CAE_OK;
        if (b) {
            HIP_TRY(hipDeviceSynchronize());
            b.reset();
        }
        return b.alloc((bytes + (1u << 20)) & ~(size_t)((1u << 20) - 1));
    }
    int ensure_device() {
        if (!flags) {
            HIP_TRY(hipHostMalloc((void **)&flags, kFlagSlots * sizeof(int), hipHostMallocMapped));
            memset(flags, 0, kFlagSlots * sizeof(int));
            HIP_TRY(hipHostGetDevicePointer((void **)&flags_dev, flags, 0));
        }
        return CAE_OK;
    }
    // calls on one handle use its workspaces in call order whatever stream they name (as Model::order_stream)
    int order_stream(hipStream_t stream) {
        if (last_stream_set && last_stream != (void *)stream) {
            if (!order_event) HIP_TRY(hipEventCreateWithFlags(&order_event, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(order_event, (hipStream_t)last_stream));
            HIP_TRY(hipStreamWaitEvent(stream, order_event, 0));
        }
        last_stream = (void *)stream;
        last_stream_set = true;
        return CAE_OK;
    }
    ~Seg() {
        if (order_event) (void)hipEventDestroy(order_event);
        if (flags) (void)hipHostFree(flags);
    }
};

static int padded_upload(DevBuf &dst, const float *v, int c, int cp) {
    std::vector<float> p(cp, 0.0f);
    std::copy(v, v + c, p.begin());
    return dst.upload(p);
}

static int make_layer(SegLayer &l, const char *name, int ks, int cin_a, int cin_b, int cout, bool up, const float *w,
                      const float *bias, const float *gamma, const float *beta) {
    const size_t nw = (size_t)(cin_a + cin_b) * cout * (up ? 4 : ks * ks);
    if (!w || (up && !bias)) return fail(CAE_ERR_ARG, "%s: NULL weight", name);
    if (!fits_f16(w, nw) || (gamma && !(fits_f16(gamma, cout) && fits_f16(beta, cout))))
        return fail(CAE_ERR_ARG, "%s: a weight, gamma or beta entry is outside the f16 range (|v| <= 65504, finite); "
                                 "the head has no fp32 path", name);
    l.ks = ks, l.cin_a = cin_a, l.cin_b = cin_b, l.cout = cout, l.up = up;
    const int m = seg_rows(cout, up);
    l.ct = seg_ct(m, ks), l.groups = seg_groups(m, ks), l.chunks = seg_chunks(cin_a, cin_b);
    l.cp = (cout + 7) / 8 * 8;
    CAE_TRY(l.wp.upload(pack_seg_f16(w, cin_a, cin_b, cout, ks, up)));
    if (bias) {
        std::vector<float> b((size_t)l.groups * l.ct * 32, 0.0f);
        for (int r = 0; r < m; ++r) {
            const int co = up ? r % l.cp : r;
            if (co < cout) b[r] = bias[co];
        }
        CAE_TRY(l.bias.upload(b));
    }
    l.norm = gamma != nullptr;
    if (gamma) {
        CAE_TRY(padded_upload(l.gamma, gamma, cout, l.cp));
        CAE_TRY(padded_upload(l.beta, beta, cout, l.cp));
    }
    return CAE_OK;
}

static int check_config(const cae_seg_config &c) {
    if (c.levels < 1 || c.levels > 8) return fail(CAE_ERR_ARG, "compression_level %d outside 1..8", c.levels);
    if (c.channels_bn < 1 || c.seg_channels_bn < 1 || c.num_classes < 1) return fail(CAE_ERR_ARG, "channel counts must be >= 1");
    for (int i = 0; i < c.levels; ++i) {
        if (c.level_channels[i] < 1 || (c.concat_bridges && c.bridge_channels[i] < 1) ||
            (i + 1 < c.levels && c.up_channels[i] < 1))
            return fail(CAE_ERR_ARG, "level %d: channel counts must be >= 1", i);
        if (i + 1 < c.levels && c.up_channels[i] != c.level_channels[i + 1])
            return fail(CAE_ERR_ARG, "level %d hands %d channels to a level of %d", i, c.up_channels[i], c.level_channels[i + 1]);
    }
    return CAE_OK;
}

}  // namespace cae

using namespace cae;

extern "C" {

int cae_seg_weight_count(const cae_seg_config *c) {
    if (!c) return fail(CAE_ERR_ARG, "NULL config");
    const int nb = c->batch_norm ? 2 : 0;
    int k = (1 + nb) * 2 + 2;  // bottleneck
    for (int i = 0; i < c->levels; ++i) k += (c->concat_bridges ? nb + 1 + nb : 0) + (1 + nb) * 2 + (i + 1 < c->levels ? 2 : 0);
    return k + 2;
}

int cae_seg_create(const cae_seg_config *cfg, const float *const *weights, int n_weights, cae_seg_t **out) {
    if (!cfg || !weights || !out) return fail(CAE_ERR_ARG, "NULL argument");
    CAE_TRY(check_config(*cfg));
    if (n_weights != cae_seg_weight_count(cfg))
        return fail(CAE_ERR_ARG, "%d weight arrays given, this configuration has %d", n_weights, cae_seg_weight_count(cfg));
    for (int i = 0; i < n_weights; ++i)
        if (!weights[i]) return fail(CAE_ERR_ARG, "weight array %d is NULL", i);
    Seg *s = new (std::nothrow) Seg;
    if (!s) return fail(CAE_ERR_NOMEM, "out of memory");
    s->cfg = *cfg;
    const cae_seg_config &c = s->cfg;
    const bool bn = c.batch_norm != 0;
    int k = 0, rc = CAE_OK;
    auto next = [&]() { return weights[k++]; };
    auto conv = [&](const char *name, int ks, int ca, int cb, int co, bool has_norm) {
        if (rc) return;
        const float *w = next(), *g = nullptr, *b = nullptr;
        if (has_norm && bn) g = next(), b = next();
        s->st.emplace_back();
        rc = make_layer(s->st.back(), name, ks, ca, cb, co, false, w, nullptr, g, b);
    };
    auto biased = [&](const char *name, int ci, int co, bool up) {
        if (rc) return;
        const float *w = next(), *b = next();
        s->st.emplace_back();
        rc = make_layer(s->st.back(), name, 1, ci, 0, co, up, w, b, nullptr, nullptr);
    };
    conv("bottleneck._c1", 1, c.channels_bn, 0, c.seg_channels_bn, true);
    conv("bottleneck._c2", 3, c.seg_channels_bn, 0, c.seg_channels_bn, true);
    biased("bottleneck._up_sample", c.seg_channels_bn, c.level_channels[0], true);
    for (int i = 0; i < c.levels && !rc; ++i) {
        const int ch = c.level_channels[i];
        if (c.concat_bridges) {
            if (bn) {
                const float *g = next(), *b = next();
                if (!fits_f16(g, c.bridge_channels[i]) || !fits_f16(b, c.bridge_channels[i]))
                    rc = fail(CAE_ERR_ARG, "bridges_projection.%d._bn1: gamma or beta outside the f16 range (|v| <= 65504)", i);
                const int cp = (c.bridge_channels[i] + 7) / 8 * 8;
                if (!rc) rc = padded_upload(s->proj_gamma[i], g, c.bridge_channels[i], cp);
                if (!rc) rc = padded_upload(s->proj_beta[i], b, c.bridge_channels[i], cp);
            }
            conv("bridges_projection._c2", 3, c.bridge_channels[i], 0, ch, true);
        }
        conv("synthesis_track._c1", 3, c.concat_bridges ? ch : 0, ch, ch, true);
        conv("synthesis_track._c2", 3, ch, 0, ch, true);
        if (i + 1 < c.levels) biased("synthesis_track._up_sample", ch, c.up_channels[i], true);
    }
    biased("fc", c.level_channels[c.levels - 1], c.num_classes, false);
    if (rc) {
        delete s;
        return rc;
    }
    *out = reinterpret_cast<cae_seg_t *>(s);
    return CAE_OK;
}

void cae_seg_destroy(cae_seg_t *h) { delete reinterpret_cast<Seg *>(h); }

int cae_seg_stage_count(cae_seg_t *h) {
    Seg *s = reinterpret_cast<Seg *>(h);
    return s ? (int)s->st.size() : fail(CAE_ERR_ARG, "NULL handle");
}

int64_t cae_seg_last_ticket(void) { return g_seg_ticket; }

int cae_seg_range_check(cae_seg_t *h, int64_t ticket) {
    Seg *s = reinterpret_cast<Seg *>(h);
    if (!s) return fail(CAE_ERR_ARG, "NULL handle");
    std::lock_guard<std::mutex> lk(s->mu);
    if (ticket <= 0 || ticket > s->flag_seq || !s->flags) return fail(CAE_ERR_ARG, "unknown range ticket");
    if (s->flag_seq - ticket >= Seg::kFlagSlots) return fail(CAE_ERR_ARG, "range ticket too old (%d calls are tracked)", Seg::kFlagSlots);
    if (*(volatile int *)(s->flags + ticket % Seg::kFlagSlots) != 0)
        return fail(CAE_ERR_RANGE, "segmentation head: a staged activation left the valid range of the f16x3 kernels "
                                   "(finite, |v| <= 65504); the head has no fp32 path yet and the logits of this call are invalid");
    return CAE_OK;
}

int cae_seg_forward(cae_seg_t *h, const float *latents_dev, const float *const *bridges_dev, int n, int lh, int lw,
                    float *logits_dev, const cae_seg_taps *taps, void *stream) {
    Seg *s = reinterpret_cast<Seg *>(h);
    if (!s || !latents_dev || !logits_dev) return fail(CAE_ERR_ARG, "NULL argument");
    const cae_seg_config &c = s->cfg;
    const int L = c.levels;
    if (n < 1 || lh < 1 || lw < 1) return fail(CAE_ERR_ARG, "n, lh, lw must be >= 1 (got %d, %d, %d)", n, lh, lw);
    if (((long)lh << L) * ((long)lw << L) > INT_MAX) return fail(CAE_ERR_ARG, "output plane of more than 2^31 - 1 pixels");
    if (c.concat_bridges) {
        if (!bridges_dev) return fail(CAE_ERR_ARG, "this head concatenates bridges: bridges_dev is NULL");
        for (int i = 0; i < L; ++i)
            if (!bridges_dev[i]) return fail(CAE_ERR_ARG, "bridge %d is NULL", i);
    }
    if (taps && (!taps->raw || !taps->ab || (c.concat_bridges && !taps->bridge_ab))) return fail(CAE_ERR_ARG, "NULL tap list");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(s->mu);
    CAE_TRY(s->ensure_device());
    CAE_TRY(s->order_stream(st));

    // workspace sizes: the largest extent each buffer takes
    auto c8 = [&](int ch, size_t hw) { return (size_t)n * ((ch + 7) / 8) * hw * 32; };
    size_t need[Seg::NWS] = {0}, cpmax = (c.seg_channels_bn + 7) / 8 * 8;
    const size_t hw0 = (size_t)lh * lw;
    need[Seg::X0] = c8(c.channels_bn, hw0);
    need[Seg::T1] = need[Seg::T2] = c8(c.seg_channels_bn, hw0);
    auto tiles_of = [](int hh, int ww) { return (size_t)((hh + SEG_TY - 1) / SEG_TY) * ((ww + SEG_TX - 1) / SEG_TX); };
    need[Seg::STATS] = tiles_of(lh, lw) * n * cpmax * 12;
    for (int i = 0; i < L; ++i) {
        const size_t hw = hw0 << (2 * (i + 1));
        const int ch = c.level_channels[i];
        need[Seg::U] = std::max(need[Seg::U], c8(ch, hw));
        need[Seg::T1] = std::max(need[Seg::T1], c8(ch, hw));
        need[Seg::T2] = std::max(need[Seg::T2], c8(ch, hw));
        size_t cpl = (ch + 7) / 8 * 8;
        if (c.concat_bridges) {
            need[Seg::BC] = std::max(need[Seg::BC], c8(c.bridge_channels[i], hw));
            need[Seg::RP] = std::max(need[Seg::RP], c8(ch, hw));
            cpmax = std::max(cpmax, (size_t)(c.bridge_channels[i] + 7) / 8 * 8);
        }
        cpmax = std::max(cpmax, cpl);
        need[Seg::STATS] = std::max(need[Seg::STATS], tiles_of(lh << (i + 1), lw << (i + 1)) * n * cpl * 12);
    }
    const size_t ab_floats = (size_t)n * cpmax * 2;
    need[Seg::AB] = 4 * ab_floats * sizeof(float);
    for (int w = 0; w < Seg::NWS; ++w)
        if (need[w]) CAE_TRY(s->ensure_ws(w, need[w]));

    const int64_t ticket = ++s->flag_seq;
    *(volatile int *)(s->flags + ticket % Seg::kFlagSlots) = 0;
    g_seg_ticket = ticket;
    int *flag = s->flags_dev + ticket % Seg::kFlagSlots;

    float *ab1 = s->ws[Seg::AB].get<float>(), *ab2 = ab1 + ab_floats, *abb = ab2 + ab_floats, *abp = abb + ab_floats;
    int stage = 0;
    // one convolution: its launch, its statistics -> (a, b) for the consumer, its taps
    auto run = [&](SegSrc A, SegSrc B, float *dst, int outmode, int hh, int ww, float *ab_out) -> int {
        SegLayer &l = s->st[stage];
        SegConvArgs a{};
        a.A = A, a.B = B;
        a.wp = l.wp.get<char>(), a.bias = l.bias.get<float>(), a.out = dst, a.flag = flag;
        a.stats = (ab_out && l.norm) ? s->ws[Seg::STATS].get<float>() : nullptr;
        a.N = n, a.H = hh, a.W = ww, a.chunks = l.chunks, a.cout = l.cout, a.out_planes = l.cp / 8, a.outmode = outmode;
        CAE_TRY(launch_seg_conv(l.ks, l.ct, l.groups, a, st));
        if (ab_out)
            CAE_TRY(launch_seg_finalize(a.stats, (int)tiles_of(hh, ww), n, l.cp, l.norm ? l.gamma.get<float>() : nullptr,
                                        l.beta.get<float>(), ab_out, st));
        if (taps) {
            const size_t ohw = (size_t)hh * ww * (outmode == SEG_OUT_SHUFFLE ? 4 : 1);
            if (taps->raw[stage]) {
                if (outmode == SEG_OUT_NCHW)
                    HIP_TRY(hipMemcpyAsync(taps->raw[stage], dst, (size_t)n * l.cout * ohw * 4, hipMemcpyDeviceToDevice, st));
                else
                    CAE_TRY(launch_seg_c8_to_nchw(dst, taps->raw[stage], n, l.cout, ohw, st));
            }
            if (ab_out && taps->ab[stage])
                HIP_TRY(hipMemcpyAsync(taps->ab[stage], ab_out, (size_t)n * l.cp * 8, hipMemcpyDeviceToDevice, st));
        }
        ++stage;
        return CAE_OK;
    };
    auto planes = [](int ch) { return (ch + 7) / 8; };
    const SegSrc none{nullptr, nullptr, 0};
    float *x0 = s->ws[Seg::X0].get<float>(), *t1 = s->ws[Seg::T1].get<float>(), *t2 = s->ws[Seg::T2].get<float>();
    float *u = s->ws[Seg::U].get<float>(), *bc = s->ws[Seg::BC].get<float>(), *rp = s->ws[Seg::RP].get<float>();

    CAE_TRY(launch_seg_nchw_to_c8(latents_dev, x0, n, c.channels_bn, hw0, st));
    CAE_TRY(run(SegSrc{x0, nullptr, planes(c.channels_bn)}, none, t1, SEG_OUT_C8, lh, lw, ab1));
    CAE_TRY(run(SegSrc{t1, ab1, planes(c.seg_channels_bn)}, none, t2, SEG_OUT_C8, lh, lw, ab2));
    CAE_TRY(run(SegSrc{t2, ab2, planes(c.seg_channels_bn)}, none, u, SEG_OUT_SHUFFLE, lh, lw, nullptr));
    for (int i = 0; i < L; ++i) {
        const int hh = lh << (i + 1), ww = lw << (i + 1), ch = c.level_channels[i];
        const size_t hw = (size_t)hh * ww;
        const SegSrc up{u, nullptr, planes(ch)};
        if (c.concat_bridges) {
            const int bch = c.bridge_channels[i];
            CAE_TRY(launch_seg_nchw_to_c8(bridges_dev[i], bc, n, bch, hw, st));
            CAE_TRY(launch_seg_plane_moments(bridges_dev[i], n, bch, planes(bch) * 8, hw, s->proj_gamma[i].get<float>(),
                                             s->proj_beta[i].get<float>(), abb, st));
            if (taps && taps->bridge_ab[i])
                HIP_TRY(hipMemcpyAsync(taps->bridge_ab[i], abb, (size_t)n * planes(bch) * 64, hipMemcpyDeviceToDevice, st));
            CAE_TRY(run(SegSrc{bc, abb, planes(bch)}, none, rp, SEG_OUT_C8, hh, ww, abp));
            CAE_TRY(run(SegSrc{rp, abp, planes(ch)}, up, t1, SEG_OUT_C8, hh, ww, ab1));
        } else {
            CAE_TRY(run(SegSrc{nullptr, nullptr, 0}, up, t1, SEG_OUT_C8, hh, ww, ab1));
        }
        CAE_TRY(run(SegSrc{t1, ab1, planes(ch)}, none, t2, SEG_OUT_C8, hh, ww, ab2));
        if (i + 1 < L) CAE_TRY(run(SegSrc{t2, ab2, planes(ch)}, none, u, SEG_OUT_SHUFFLE, hh, ww, nullptr));
    }
    return run(SegSrc{t2, ab2, planes(c.level_channels[L - 1])}, none, logits_dev, SEG_OUT_NCHW, lh << L, lw << L, nullptr);
}

int cae_seg_set_weights(cae_seg_t *h, const float *const *weights_dev, int n_weights, void *stream) {
    Seg *s = reinterpret_cast<Seg *>(h);
    if (!s || !weights_dev) return fail(CAE_ERR_ARG, "NULL argument");
    const cae_seg_config &c = s->cfg;
    if (n_weights != cae_seg_weight_count(&c))
        return fail(CAE_ERR_ARG, "%d weight arrays given, this configuration has %d", n_weights, cae_seg_weight_count(&c));
    for (int i = 0; i < n_weights; ++i)
        if (!weights_dev[i]) return fail(CAE_ERR_ARG, "weight array %d is NULL", i);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(s->mu);
    CAE_TRY(s->ensure_device());
    CAE_TRY(s->order_stream(st));
    const int64_t ticket = ++s->flag_seq;
    *(volatile int *)(s->flags + ticket % Seg::kFlagSlots) = 0;
    g_seg_ticket = ticket;
    int *flag = s->flags_dev + ticket % Seg::kFlagSlots;
    const bool bn = c.batch_norm != 0;
    int k = 0, stage = 0;
    // (the walk of cae_seg_create)
    auto layer = [&](bool biased) -> int {
        SegLayer &l = s->st[stage++];
        CAE_TRY(launch_seg_pack_dev(weights_dev[k++], l.cin_a, l.cin_b, l.cout, l.ks, l.up, l.wp.get<char>(), flag, st));
        if (biased) CAE_TRY(launch_seg_pad_vec(weights_dev[k++], l.cout, l.up, l.groups * l.ct * 32, false, l.bias.get<float>(), flag, st));
        if (l.norm) {
            CAE_TRY(launch_seg_pad_vec(weights_dev[k++], l.cout, false, l.cp, true, l.gamma.get<float>(), flag, st));
            CAE_TRY(launch_seg_pad_vec(weights_dev[k++], l.cout, false, l.cp, true, l.beta.get<float>(), flag, st));
        }
        return CAE_OK;
    };
    CAE_TRY(layer(false));
    CAE_TRY(layer(false));
    CAE_TRY(layer(true));
    for (int i = 0; i < c.levels; ++i) {
        if (c.concat_bridges) {
            if (bn) {
                const int bc = c.bridge_channels[i], cp = (bc + 7) / 8 * 8;
                CAE_TRY(launch_seg_pad_vec(weights_dev[k++], bc, false, cp, true, s->proj_gamma[i].get<float>(), flag, st));
                CAE_TRY(launch_seg_pad_vec(weights_dev[k++], bc, false, cp, true, s->proj_beta[i].get<float>(), flag, st));
            }
            CAE_TRY(layer(false));
        }
        CAE_TRY(layer(false));
        CAE_TRY(layer(false));
        if (i + 1 < c.levels) CAE_TRY(layer(true));
    }
    return layer(true);
}

void cae_seg_tile(int *tx, int *ty) {
    if (tx) *tx = SEG_TX;
    if (ty) *ty = SEG_TY;
}

}  // extern "C"
