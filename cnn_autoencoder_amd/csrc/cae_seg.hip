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

// One convolution of the head as seg_plan states it from the config alone: the public record (include/cae_hip.h) and
// where the stage runs.  Every walk over the head is a loop over these.
struct SegStage : cae_seg_stage_info {
    char name[48];          // the reference's state-dict name with the level index, "synthesis_track.1._c2"
    int src_a, src_b, dst;  // Seg::X0 .. RP; -1: no such source / the caller's logits.  A bridge is staged into src_a first
    int ab_r, ab_w;         // the Seg::AB1 .. ABP slot source A is read through / this stage's statistics go to; -1: none
    int outmode, shift;     // SEG_OUT_*; the stage's input planes are (lh << shift, lw << shift)
};

// The device side of one stage: packed weight, bias rows, the gamma / beta of the GroupNorm behind it (batch_norm only)
struct SegLayer {
    int ct = 1, groups = 1, chunks = 1, cp = 8;  // cp: channels of the output's plane grid
    DevBuf wp, bias;
    DevBuf gamma, beta;  // [cp], zero padded
};

struct Seg {
    cae_seg_config cfg;
    std::vector<SegStage> plan;  // in launch order
    std::vector<SegLayer> st;    // one per stage
    DevBuf proj_gamma[8], proj_beta[8];  // the _bn1 in front of a bridge's stage (on the bridges)
    enum { X0, T1, T2, U, BC, RP, AB, STATS, NWS };  // workspaces
    enum { AB1, AB2, ABB, ABP, NSLOTS };             // the (a, b) slots inside AB
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
    // a fresh range ticket for this thread's call (after ensure_device) -> the device word its launches raise
    int *draw_ticket() {
        const int64_t ticket = ++flag_seq;
        *(volatile int *)(flags + ticket % kFlagSlots) = 0;
        g_seg_ticket = ticket;
        return flags_dev + ticket % kFlagSlots;
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

static int make_layer(SegLayer &l, const SegStage &p, const float *w, const float *bias, const float *gamma,
                      const float *beta) {
    const int ks = p.ks, cin_a = p.cin_a, cin_b = p.cin_b, cout = p.cout;
    const bool up = p.up != 0;
    const size_t nw = (size_t)(cin_a + cin_b) * cout * (up ? 4 : ks * ks);
    if (!w || (up && !bias)) return fail(CAE_ERR_ARG, "%s: NULL weight", p.name);
    if (!fits_f16(w, nw) || (gamma && !(fits_f16(gamma, cout) && fits_f16(beta, cout))))
        return fail(CAE_ERR_ARG, "%s: a weight, gamma or beta entry is outside the f16 range (|v| <= 65504, finite); "
                                 "the head has no fp32 path", p.name);
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
    if (gamma) {
        CAE_TRY(padded_upload(l.gamma, gamma, cout, l.cp));
        CAE_TRY(padded_upload(l.beta, beta, cout, l.cp));
    }
    return CAE_OK;
}

// The head's structure, stated once (levels inside 1..8): bottleneck _c1 _c2 _up_sample, per level {projection of bridge
// i: _bn1 on the bridge, _c2} _c1 _c2 [_up_sample], fc.  The running features go T1 -> T2 -> U, a bridge BC -> RP, and RP
// is contracted in front of U by the level's _c1.
static std::vector<SegStage> seg_plan(const cae_seg_config &c) {
    std::vector<SegStage> plan;
    const int gn = c.batch_norm ? 2 : 0, L = c.levels, sbn = c.seg_channels_bn;
    auto producer = [&](int buf) {  // the latest stage that wrote `buf`; -1: the latents or a bridge, -2: no source
        int k = buf < 0 ? -2 : (int)plan.size() - 1;
        while (k >= 0 && plan[k].dst != buf) --k;
        return k;
    };
    auto add = [&](const char *unit, int level, const char *conv, int ks, int cin_a, int cin_b, int cout, int src_a, int ab_r,
                   int dst, int ab_w, int shift, int bridge = -1) {
        SegStage s{};
        if (level < 0) snprintf(s.name, sizeof s.name, "%s%s", unit, conv);
        else snprintf(s.name, sizeof s.name, "%s.%d%s", unit, level, conv);
        s.ks = ks, s.cin_a = cin_a, s.cin_b = cin_b, s.cout = cout, s.bridge = bridge, s.shift = shift;
        s.src_a = src_a, s.src_b = cin_b ? Seg::U : -1, s.dst = dst, s.ab_r = ab_r, s.ab_w = ab_w;
        s.up = dst == Seg::U, s.biased = s.up || dst < 0, s.norm = ab_w >= 0;
        s.outmode = s.up ? SEG_OUT_SHUFFLE : dst < 0 ? SEG_OUT_NCHW : SEG_OUT_C8;
        s.src_a_stage = producer(s.src_a), s.src_b_stage = producer(s.src_b), s.src_a_transformed = ab_r >= 0;
        s.n_weights = (bridge >= 0 ? gn : 0) + 1 + s.biased + (s.norm ? gn : 0);
        plan.push_back(s);
    };
    add("bottleneck", -1, "._c1", 1, c.channels_bn, 0, sbn, Seg::X0, -1, Seg::T1, Seg::AB1, 0);
    add("bottleneck", -1, "._c2", 3, sbn, 0, sbn, Seg::T1, Seg::AB1, Seg::T2, Seg::AB2, 0);
    add("bottleneck", -1, "._up_sample", 1, sbn, 0, c.level_channels[0], Seg::T2, Seg::AB2, Seg::U, -1, 0);
    for (int i = 0; i < L; ++i) {
        const int ch = c.level_channels[i], cat = c.concat_bridges;
        if (cat) add("bridges_projection", i, "._c2", 3, c.bridge_channels[i], 0, ch, Seg::BC, Seg::ABB, Seg::RP, Seg::ABP, i + 1, i);
        add("synthesis_track", i, "._c1", 3, cat ? ch : 0, ch, ch, cat ? Seg::RP : -1, cat ? Seg::ABP : -1, Seg::T1, Seg::AB1, i + 1);
        add("synthesis_track", i, "._c2", 3, ch, 0, ch, Seg::T1, Seg::AB1, Seg::T2, Seg::AB2, i + 1);
        if (i + 1 < L) add("synthesis_track", i, "._up_sample", 1, ch, 0, c.up_channels[i], Seg::T2, Seg::AB2, Seg::U, -1, i + 1);
    }
    add("fc", -1, "", 1, c.level_channels[L - 1], 0, c.num_classes, Seg::T2, Seg::AB2, -1, -1, L);
    return plan;
}

// the plan of a config, or CAE_ERR_ARG: every stage has channels, and a source has the channels its producer writes
static int checked_plan(const cae_seg_config *c, std::vector<SegStage> &plan) {
    if (!c) return fail(CAE_ERR_ARG, "NULL config");
    if (c->levels < 1 || c->levels > 8) return fail(CAE_ERR_ARG, "compression_level %d outside 1..8", c->levels);
    plan = seg_plan(*c);
    for (const SegStage &p : plan) {
        if (p.cout < 1 || (p.src_a >= 0 && p.cin_a < 1) || (p.src_b >= 0 && p.cin_b < 1))
            return fail(CAE_ERR_ARG, "%s: channel counts must be >= 1", p.name);
        if (p.src_b_stage >= 0 && plan[p.src_b_stage].cout != p.cin_b)
            return fail(CAE_ERR_ARG, "%s hands %d channels to %s, which takes %d", plan[p.src_b_stage].name,
                        plan[p.src_b_stage].cout, p.name, p.cin_b);
    }
    return CAE_OK;
}

static int plan_weights(const std::vector<SegStage> &plan) {
    int k = 0;
    for (const SegStage &p : plan) k += p.n_weights;
    return k;
}

static int check_extent(const cae_seg_config &c, int n, int lh, int lw) {
    if (n < 1 || lh < 1 || lw < 1) return fail(CAE_ERR_ARG, "n, lh, lw must be >= 1 (got %d, %d, %d)", n, lh, lw);
    if (((long)lh << c.levels) * ((long)lw << c.levels) > INT_MAX) return fail(CAE_ERR_ARG, "output plane of more than 2^31 - 1 pixels");
    return CAE_OK;
}

static size_t seg_tiles(int hh, int ww) { return (size_t)((hh + SEG_TY - 1) / SEG_TY) * ((ww + SEG_TX - 1) / SEG_TX); }

// workspace sizes: the largest extent each buffer takes over the plan -> need[]; returns the floats of one (a, b) slot
static size_t seg_workspace(const std::vector<SegStage> &plan, int n, int lh, int lw, size_t need[Seg::NWS]) {
    auto c8 = [&](int ch, size_t hw) { return (size_t)n * ((ch + 7) / 8) * hw * 32; };
    auto grow = [&](int which, size_t bytes) { if (which >= 0) need[which] = std::max(need[which], bytes); };
    size_t cpmax = 0;
    std::fill(need, need + Seg::NWS, (size_t)0);
    for (const SegStage &p : plan) {
        const int hh = lh << p.shift, ww = lw << p.shift;
        const size_t hw = (size_t)hh * ww, cp = (p.cout + 7) / 8 * 8;
        grow(p.src_a, c8(p.cin_a, hw));
        grow(p.src_b, c8(p.cin_b, hw));
        grow(p.dst, c8(p.cout, hw * (p.up ? 4 : 1)));
        if (p.bridge >= 0) cpmax = std::max(cpmax, (size_t)(p.cin_a + 7) / 8 * 8);
        if (p.norm) {
            cpmax = std::max(cpmax, cp);
            grow(Seg::STATS, seg_tiles(hh, ww) * n * cp * 12);
        }
    }
    need[Seg::AB] = Seg::NSLOTS * (size_t)n * cpmax * 2 * sizeof(float);
    return (size_t)n * cpmax * 2;
}

}  // namespace cae

using namespace cae;

extern "C" {

int cae_seg_plan(const cae_seg_config *cfg, cae_seg_stage_info *out, int capacity) {
    std::vector<SegStage> plan;
    CAE_TRY(checked_plan(cfg, plan));
    for (int k = 0; out && k < capacity && k < (int)plan.size(); ++k) out[k] = plan[k];
    return (int)plan.size();
}

int cae_seg_workspace_bytes(const cae_seg_config *cfg, int n, int lh, int lw, size_t *out) {
    std::vector<SegStage> plan;
    CAE_TRY(checked_plan(cfg, plan));
    if (!out) return fail(CAE_ERR_ARG, "NULL argument");
    CAE_TRY(check_extent(*cfg, n, lh, lw));
    seg_workspace(plan, n, lh, lw, out);
    return CAE_OK;
}

int cae_seg_weight_count(const cae_seg_config *cfg) {
    std::vector<SegStage> plan;
    CAE_TRY(checked_plan(cfg, plan));
    return plan_weights(plan);
}

int cae_seg_create(const cae_seg_config *cfg, const float *const *weights, int n_weights, cae_seg_t **out) {
    if (!cfg || !weights || !out) return fail(CAE_ERR_ARG, "NULL argument");
    std::vector<SegStage> plan;
    CAE_TRY(checked_plan(cfg, plan));
    const int want = plan_weights(plan);
    if (n_weights != want) return fail(CAE_ERR_ARG, "%d weight arrays given, this configuration has %d", n_weights, want);
    for (int i = 0; i < n_weights; ++i)
        if (!weights[i]) return fail(CAE_ERR_ARG, "weight array %d is NULL", i);
    Seg *s = new (std::nothrow) Seg;
    if (!s) return fail(CAE_ERR_NOMEM, "out of memory");
    s->cfg = *cfg;
    s->plan = std::move(plan);
    const bool bn = s->cfg.batch_norm != 0;
    const float *const *w = weights;  // consumed in the plan's order: [_bn1 gamma beta] weight [bias] [gamma beta]
    int rc = CAE_OK;
    for (const SegStage &p : s->plan) {
        if (p.bridge >= 0 && bn) {
            const float *g = *w++, *b = *w++;
            const int cp = (p.cin_a + 7) / 8 * 8;
            if (!fits_f16(g, p.cin_a) || !fits_f16(b, p.cin_a))
                rc = fail(CAE_ERR_ARG, "the _bn1 in front of %s: gamma or beta outside the f16 range (|v| <= 65504)", p.name);
            if (!rc) rc = padded_upload(s->proj_gamma[p.bridge], g, p.cin_a, cp);
            if (!rc) rc = padded_upload(s->proj_beta[p.bridge], b, p.cin_a, cp);
        }
        const float *wt = *w++, *bias = p.biased ? *w++ : nullptr, *g = nullptr, *b = nullptr;
        if (p.norm && bn) g = *w++, b = *w++;
        s->st.emplace_back();
        if (!rc) rc = make_layer(s->st.back(), p, wt, bias, g, b);
        if (rc) break;
    }
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
    return s ? (int)s->plan.size() : fail(CAE_ERR_ARG, "NULL handle");
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
    CAE_TRY(check_extent(c, n, lh, lw));
    if (c.concat_bridges) {
        if (!bridges_dev) return fail(CAE_ERR_ARG, "this head concatenates bridges: bridges_dev is NULL");
        for (int i = 0; i < c.levels; ++i)
            if (!bridges_dev[i]) return fail(CAE_ERR_ARG, "bridge %d is NULL", i);
    }
    if (taps && (!taps->raw || !taps->ab || (c.concat_bridges && !taps->bridge_ab))) return fail(CAE_ERR_ARG, "NULL tap list");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(s->mu);
    CAE_TRY(s->ensure_device());
    CAE_TRY(s->order_stream(st));

    size_t need[Seg::NWS];
    const size_t ab_floats = seg_workspace(s->plan, n, lh, lw, need);
    for (int w = 0; w < Seg::NWS; ++w)
        if (need[w]) CAE_TRY(s->ensure_ws(w, need[w]));
    int *flag = s->draw_ticket();

    auto buf = [&](int which) { return which < 0 ? nullptr : s->ws[which].get<float>(); };
    auto slot = [&](int which) { return which < 0 ? nullptr : s->ws[Seg::AB].get<float>() + which * ab_floats; };
    auto planes = [](int ch) { return (ch + 7) / 8; };
    // one convolution: its inputs staged, its launch, its statistics -> (a, b) for the consumer, its taps
    for (size_t stage = 0; stage < s->plan.size(); ++stage) {
        const SegStage &p = s->plan[stage];
        SegLayer &l = s->st[stage];
        const int hh = lh << p.shift, ww = lw << p.shift;
        const size_t hw = (size_t)hh * ww;
        float *dst = p.dst < 0 ? logits_dev : buf(p.dst), *ab_out = slot(p.ab_w);
        if (p.src_a == Seg::X0) CAE_TRY(launch_seg_nchw_to_c8(latents_dev, buf(p.src_a), n, p.cin_a, hw, st));  // the latents
        if (p.bridge >= 0) {  // the bridge, and the (a, b) pairs of the _bn1 on it
            const float *b = bridges_dev[p.bridge];
            CAE_TRY(launch_seg_nchw_to_c8(b, buf(p.src_a), n, p.cin_a, hw, st));
            CAE_TRY(launch_seg_plane_moments(b, n, p.cin_a, planes(p.cin_a) * 8, hw, s->proj_gamma[p.bridge].get<float>(),
                                             s->proj_beta[p.bridge].get<float>(), slot(p.ab_r), st));
            if (taps && taps->bridge_ab[p.bridge])
                HIP_TRY(hipMemcpyAsync(taps->bridge_ab[p.bridge], slot(p.ab_r), (size_t)n * planes(p.cin_a) * 64,
                                       hipMemcpyDeviceToDevice, st));
        }
        SegConvArgs a{};
        a.A = SegSrc{buf(p.src_a), slot(p.ab_r), planes(p.cin_a)}, a.B = SegSrc{buf(p.src_b), nullptr, planes(p.cin_b)};
        a.wp = l.wp.get<char>(), a.bias = l.bias.get<float>(), a.out = dst, a.flag = flag;
        a.stats = (ab_out && l.gamma) ? s->ws[Seg::STATS].get<float>() : nullptr;
        a.N = n, a.H = hh, a.W = ww, a.chunks = l.chunks, a.cout = p.cout, a.out_planes = l.cp / 8, a.outmode = p.outmode;
        CAE_TRY(launch_seg_conv(p.ks, l.ct, l.groups, a, st));
        if (ab_out)  // (without batch_norm too: no statistics, no gamma -> the identity pairs)
            CAE_TRY(launch_seg_finalize(a.stats, (int)seg_tiles(hh, ww), n, l.cp, l.gamma.get<float>(), l.beta.get<float>(),
                                        ab_out, st));
        if (taps) {
            const size_t ohw = hw * (p.up ? 4 : 1);
            if (taps->raw[stage]) {
                if (p.dst < 0)
                    HIP_TRY(hipMemcpyAsync(taps->raw[stage], dst, (size_t)n * p.cout * ohw * 4, hipMemcpyDeviceToDevice, st));
                else
                    CAE_TRY(launch_seg_c8_to_nchw(dst, taps->raw[stage], n, p.cout, ohw, st));
            }
            if (ab_out && taps->ab[stage])
                HIP_TRY(hipMemcpyAsync(taps->ab[stage], ab_out, (size_t)n * l.cp * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    return CAE_OK;
}

int cae_seg_set_weights(cae_seg_t *h, const float *const *weights_dev, int n_weights, void *stream) {
    Seg *s = reinterpret_cast<Seg *>(h);
    if (!s || !weights_dev) return fail(CAE_ERR_ARG, "NULL argument");
    const int want = plan_weights(s->plan);
    if (n_weights != want) return fail(CAE_ERR_ARG, "%d weight arrays given, this configuration has %d", n_weights, want);
    for (int i = 0; i < n_weights; ++i)
        if (!weights_dev[i]) return fail(CAE_ERR_ARG, "weight array %d is NULL", i);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(s->mu);
    CAE_TRY(s->ensure_device());
    CAE_TRY(s->order_stream(st));
    int *flag = s->draw_ticket();
    const float *const *w = weights_dev;  // consumed as cae_seg_create consumes the host arrays
    for (size_t stage = 0; stage < s->plan.size(); ++stage) {
        const SegStage &p = s->plan[stage];
        SegLayer &l = s->st[stage];
        if (p.bridge >= 0 && s->cfg.batch_norm) {
            const int cp = (p.cin_a + 7) / 8 * 8;
            CAE_TRY(launch_seg_pad_vec(*w++, p.cin_a, false, cp, true, s->proj_gamma[p.bridge].get<float>(), flag, st));
            CAE_TRY(launch_seg_pad_vec(*w++, p.cin_a, false, cp, true, s->proj_beta[p.bridge].get<float>(), flag, st));
        }
        CAE_TRY(launch_seg_pack_dev(*w++, p.cin_a, p.cin_b, p.cout, p.ks, p.up != 0, l.wp.get<char>(), flag, st));
        if (p.biased) CAE_TRY(launch_seg_pad_vec(*w++, p.cout, p.up != 0, l.groups * l.ct * 32, false, l.bias.get<float>(), flag, st));
        if (l.gamma) {
            CAE_TRY(launch_seg_pad_vec(*w++, p.cout, false, l.cp, true, l.gamma.get<float>(), flag, st));
            CAE_TRY(launch_seg_pad_vec(*w++, p.cout, false, l.cp, true, l.beta.get<float>(), flag, st));
        }
    }
    return CAE_OK;
}

void cae_seg_tile(int *tx, int *ty) {
    if (tx) *tx = SEG_TX;
    if (ty) *ty = SEG_TY;
}

}  // extern "C"
