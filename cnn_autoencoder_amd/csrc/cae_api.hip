// Host side of libcae_hip.so: model handle, weight packing, kernel dispatch (see include/cae_hip.h).
#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_kernels.hpp"
#include "cae_kernels_f16.hpp"
#include "cae_launch.hpp"
#include "cae_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace cae {

thread_local std::string g_last_error;
thread_local int64_t g_last_ticket = 0;  // range ticket of this thread's latest analysis / synthesis call (0: fp32 call)
thread_local int g_force_fp32 = 0;       // cae_thread_force_fp32

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

void dev_free(void *p) { (void)hipFree(p); }

int DevBuf::alloc(size_t n) {
    reset();
    HIP_TRY(hipMalloc(&p, n));
    bytes = n;
    return CAE_OK;
}

int DevBuf::upload(const void *src, size_t n) {
    CAE_TRY(alloc(n));
    HIP_TRY(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    return CAE_OK;
}

int Model::ensure_ws(int which, size_t bytes) {
    DevBuf &b = ws[which];
    if (b.bytes >= bytes) return CAE_OK;
    if (b) {
        HIP_TRY(hipDeviceSynchronize());
        b.reset();
    }
    return b.alloc((bytes + (1u << 20)) & ~(size_t)((1u << 20) - 1));
}

int Model::order_stream(void *stream) {
    if (last_stream_set && last_stream != stream) {
        if (!order_event) HIP_TRY(hipEventCreateWithFlags((hipEvent_t *)&order_event, hipEventDisableTiming));
        HIP_TRY(hipEventRecord((hipEvent_t)order_event, (hipStream_t)last_stream));
        HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)order_event, 0));
    }
    last_stream = stream;
    last_stream_set = true;
    return CAE_OK;
}

int Model::ensure_device() {
    if (!zero) {
        CAE_TRY(zero.alloc(1024));  // zero page: out-of-range halo source, null medians (192 floats)
        HIP_TRY(hipMemset(zero.p, 0, 1024));
    }
    if (medians_dirty && ent.channels > 0) {
        CAE_TRY(medians_dev.upload(ent.medians));
        medians_dirty = false;
    }
    if (density_dirty && !density.empty()) {
        CAE_TRY(density_dev.upload(density));
        density_dirty = false;
    }
    if (!flags) {
        HIP_TRY(hipHostMalloc((void **)&flags, kFlagSlots * sizeof(int), hipHostMallocMapped));
        memset(flags, 0, kFlagSlots * sizeof(int));
        HIP_TRY(hipHostGetDevicePointer((void **)&flags_dev, flags, 0));
    }
    return CAE_OK;
}

int *Model::next_flag(int64_t *ticket) {
    *ticket = ++flag_seq;
    const int slot = (int)(*ticket % kFlagSlots);
    *(volatile int *)(flags + slot) = 0;  // the word's previous user was kFlagSlots calls ago
    g_last_ticket = *ticket;
    return flags_dev + slot;
}

bool Model::f16_usable() const {
    if (precision != 1 || g_force_fp32) return false;
    for (auto *tr : {&enc, &dec})
        for (auto &l : *tr)
            if (l.set && l.f16_bad) return false;
    return true;
}

Model::~Model() {  // (every device buffer frees itself)
    if (order_event) (void)hipEventDestroy((hipEvent_t)order_event);
    if (flags) (void)hipHostFree(flags);
}

// ---- kernel dispatch ---------------------------------------------------------------------------
struct ProfScope {
    Model *m;
    int track;
    hipStream_t st;
    std::vector<std::pair<void *, void *>> ev;
    hipEvent_t cur = nullptr;
    ProfScope(Model *m_, int track_, hipStream_t st_) : m(m_), track(track_), st(st_) {}
    void begin() {
        if (!m->profiling) return;
        hipEvent_t a;
        if (hipEventCreate(&a) != hipSuccess) return;
        (void)hipEventRecord(a, st);
        cur = a;
    }
    void end() {
        if (!m->profiling || !cur) return;
        hipEvent_t b;
        if (hipEventCreate(&b) != hipSuccess) return;
        (void)hipEventRecord(b, st);
        ev.emplace_back((void *)cur, (void *)b);
        cur = nullptr;
    }
    ~ProfScope() {
        if (m->profiling && !ev.empty()) m->prof[track].push_back(std::move(ev));
    }
};

static unsigned ew_grid(size_t total) {
    size_t b = (total + 255) / 256;
    return (unsigned)std::min<size_t>(std::max<size_t>(b, 1), 256 * 8 * 4);
}

// The layer a (track, index) pair names, into `l`.
static int layer_of(Model *m, int track, int index, Layer *&l) {
    if (track != CAE_ANALYSIS && track != CAE_SYNTHESIS) return fail(CAE_ERR_ARG, "bad track %d", track);
    if (index < 0 || index >= m->L) return fail(CAE_ERR_ARG, "layer index %d out of range", index);
    l = &(track == CAE_ANALYSIS ? m->enc : m->dec)[index];
    return CAE_OK;
}

// A per-channel vector (bias: fill 0, beta: fill 1) padded to ct*32 entries on the device; no vector, no buffer.
static int upload_channels(DevBuf &d, const float *v, int c, int ct, float fill) {
    if (!v) {
        d.reset();
        return CAE_OK;
    }
    // The kernels read these vectors as 16-byte pieces, whole channel tiles at a time (load_acc_tile, cae_kernels.hpp):
    // the host vector `v` may lie anywhere, its padded copy is an allocation of its own -- ct * 32 floats at an address
    // hipMalloc aligns to 256 bytes.  Checked, not assumed: a buffer that broke this would fault in the kernel.
    CAE_TRY(d.upload(pad_channels(v, c, ct, fill)));
    if ((uintptr_t)d.p % 16 != 0 || d.bytes != (size_t)ct * 32 * sizeof(float))
        return fail(CAE_ERR_HIP, "per-channel vector: device buffer %p (%zu bytes) is not a 16-byte aligned run of %d floats",
                    d.p, d.bytes, ct * 32);
    return CAE_OK;
}

// What every launch site fills the same way; the site adds its weights and whatever else is special about it.  (Tile
// grid and contraction chunks are the launcher's business: cae_launch_*.hip.)
static LayerArgs layer_args(const Model *m, const float *in, int in_planes, void *out, int n, int h, int w, int oh, int ow,
                            int ct, int cout, int outfmt, int act, int *flag) {
    LayerArgs a{};
    a.in = in;
    a.out = out;
    a.zero = m->zero.get<float>();
    a.medians = m->zero.get<float>();
    a.flag = flag;
    a.N = n;
    a.H = h;
    a.W = w;
    a.OH = oh;
    a.OW = ow;
    a.in_planes = in_planes;
    a.out_planes = ct * 4;
    a.cout = cout;
    a.outfmt = outfmt;
    a.act = act;
    return a;
}

}  // namespace cae

using namespace cae;

template <int R>
static void launch_likelihood(Model *m, const float *y, int n, int hw, float *yhat, float *lik, double *part,
                              hipStream_t st) {
    hipLaunchKernelGGL(likelihood_kernel<R>, dim3(m->c_bn, n), dim3(256), 0, st, y, m->medians_dev.get<float>(),
                       m->density_dev.get<float>(), m->density_per_channel, m->density_k, m->density_bound,
                       m->likelihood_plain, m->c_bn, hw, yhat, lik, part);
}

// (re)builds stage `stage` of a unit: a stride-1 (transposed) convolution cin -> cin with its epilogue
static int set_stage(Model *m, int track, Layer &l, int stage, const float *w, const float *bias, const float *beta,
                     const float *gamma, int act, int add_residual, int post_act) {
    const int ctin = round_ct(l.cin);
    if (ctin < 0) return fail(CAE_ERR_UNSUPPORTED, "more than 192 channels not supported");
    if ((int)l.stages.size() <= stage) l.stages.resize(stage + 1);
    Layer::Stage &sg = l.stages[stage];
    // synthesis: ConvTranspose2d(stride 1, padding k//2) == zero-padded correlation with the flipped kernel
    const bool tr = track == CAE_SYNTHESIS;
    CAE_TRY(sg.wp.upload(pack_weights(w, tr, l.cin, l.cin, m->ks, ctin, tr)));
    CAE_TRY(upload_channels(sg.bias, bias, l.cin, ctin, 0.0f));
    sg.gdn = beta != nullptr;
    if (sg.gdn) {
        CAE_TRY(upload_channels(sg.beta, beta, l.cin, ctin, 1.0f));
        CAE_TRY(sg.gp.upload(pack_gamma(gamma, l.cin, ctin)));
    }
    sg.act = act;
    sg.add_res = add_residual != 0;
    sg.post_act = post_act;
    if (m->precision == 1) {  // f16x3: the stage's weights as split halves (same packing as the strided layers)
        if (!fits_f16(w, (size_t)l.cin * l.cin * m->ks * m->ks)) l.f16_bad = true;
        CAE_TRY(sg.wp16.upload(pack_weights_f16(w, tr, l.cin, l.cin, m->ks, ctin, tr)));
        if (sg.gdn) {
            if (!fits_f16(gamma, (size_t)l.cin * l.cin)) l.f16_bad = true;
            CAE_TRY(sg.gp16.upload(pack_gamma_f16(gamma, l.cin, ctin)));
        }
    }
    if (track == CAE_ANALYSIS) {  // the fused first-layer kernels read the raw tile; a stage sits in between
        l.wp_edge.reset();
        l.wp_edge16.reset();
    }
    return CAE_OK;
}

// Runs the stride-1 stages of a unit.  `cur`/`cur_idx`: the unit's input and the workspace slot it lives in; on
// return they describe the strided layer's input.  Slots 1..3 rotate so that the unit input survives until the
// residual sum has read it.
static int pick_slot(int a, int b) {
    for (int k = 1; k <= 3; ++k)
        if (k != a && k != b) return k;
    return 1;
}

// The split-f16 stride-1 kernel carries the (I)GDN / residual-sum epilogue up to 128 channels (registers); a wider unit
// takes its stages on the fp32 kernels, between two layout conversions.
static bool stages_need_fp32(const Layer &l) {
    if (round_ct(l.cin) <= 4) return false;
    for (const Layer::Stage &sg : l.stages)
        if (sg.gdn || sg.add_res || sg.post_act) return true;
    return false;
}

// f16: the split-f16 kernels (activation stages up to 192 channels; GDN / residual stages up to 128)
static int run_stages(Model *m, const Layer &l, bool synthesis, int n, int ch, int cw, const float *&cur, int &cur_idx,
                      int &cur_planes, hipStream_t st, bool f16 = false, int *flag = nullptr) {
    if (f16 && stages_need_fp32(l)) {
        // split rows -> fp32 C8 (the unit input is dead afterwards), the stages on the fp32 kernels, fp32 C8 -> split rows
        const int tmp = pick_slot(cur_idx, cur_idx);
        const size_t rows = (size_t)n * cur_planes * ch;
        if (synthesis)
            hipLaunchKernelGGL(c8s_to_c8_kernel<true>, dim3(ew_grid(rows * cw)), dim3(256), 0, st, (const char *)cur,
                               (float *)m->ws[tmp].p, rows, cw);
        else
            hipLaunchKernelGGL(c8s_to_c8_kernel<false>, dim3(ew_grid(rows * cw)), dim3(256), 0, st, (const char *)cur,
                               (float *)m->ws[tmp].p, rows, cw);
        HIP_TRY(hipGetLastError());
        cur = (const float *)m->ws[tmp].p;
        cur_idx = tmp;
        int rc = run_stages(m, l, synthesis, n, ch, cw, cur, cur_idx, cur_planes, st, false, nullptr);
        if (rc) return rc;
        const int back = pick_slot(cur_idx, cur_idx);
        const size_t orows = (size_t)n * cur_planes * ch;
        if (synthesis)
            hipLaunchKernelGGL(c8_to_c8s_kernel<true>, dim3(ew_grid(orows * cw)), dim3(256), 0, st, cur, (char *)m->ws[back].p,
                               orows, cw, flag);
        else
            hipLaunchKernelGGL(c8_to_c8s_kernel<false>, dim3(ew_grid(orows * cw)), dim3(256), 0, st, cur, (char *)m->ws[back].p,
                               orows, cw, flag);
        HIP_TRY(hipGetLastError());
        cur = (const float *)m->ws[back].p;
        cur_idx = back;
        return CAE_OK;
    }
    const float *unit_in = cur;
    const int unit_idx = cur_idx, unit_planes = cur_planes;
    for (const Layer::Stage &sg : l.stages) {
        const int ctin = round_ct(l.cin);
        const int out_idx = pick_slot(unit_idx, cur_idx);
        LayerArgs b = layer_args(m, cur, cur_planes, m->ws[out_idx].p, n, ch, cw, ch, cw, ctin, l.cin, OUT_C8, sg.act,
                                 f16 ? flag : nullptr);
        b.bias = sg.bias.get<float>();
        b.beta = sg.beta.get<float>();
        b.res = sg.add_res ? unit_in : nullptr;
        b.res_planes = unit_planes;
        b.post_act = sg.post_act;
        int rc;
        if (f16) {
            if (!sg.wp16 || (sg.gdn && !sg.gp16)) return fail(CAE_ERR_ARG, "stage uploaded before precision 1 was selected");
            b.wp = sg.wp16.get<float>();
            b.gp = sg.gp16.get<float>();
            rc = launch_conv_s1_f16(m->ks, ctin, synthesis, sg.gdn, l.cin, b, st);
        } else {
            b.wp = sg.wp.get<float>();
            b.gp = sg.gp.get<float>();
            rc = launch_conv_s1(m->ks, ctin, synthesis, sg.gdn, l.cin, b, st);
        }
        if (rc) return rc;
        cur = (const float *)b.out;
        cur_idx = out_idx;
        cur_planes = ctin * 4;
    }
    return CAE_OK;
}

// Colour layer of a synthesis level: the reflect-padded stride-1 convolution of the level's activations `in` (h x w,
// fp32 C8 rows, or C8SP split rows on the f16x3 path) to its image channels, fp32 NCHW in `out`.
static int launch_color(Model *m, const Layer &l, bool f16, const float *in, int in_planes, int n, int h, int w, float *out,
                        int *flag, hipStream_t st) {
    const int ct = round_ct(l.color_cout);
    LayerArgs c = layer_args(m, in, in_planes, out, n, h, w, h, w, ct, l.color_cout, OUT_NCHW, 0, f16 ? flag : nullptr);
    c.bias = l.color_bias.get<float>();
    if (f16) {
        c.wp = l.color_wp16.get<float>();
        return launch_color_f16(m->ks, l.cout, c, st);
    }
    c.wp = l.color_wp.get<float>();
    return launch_conv_s1(m->ks, ct, false, false, l.cout, c, st);
}

extern "C" {

int cae_version(void) { return 1; }
const char *cae_last_error(void) { return g_last_error.c_str(); }
void cae_free(void *p) { free(p); }

int cae_model_create(int channels_org, int channels_net, int channels_bn, int compression_level, int kernel_size,
                     cae_model_t **out) {
    if (!out) return fail(CAE_ERR_ARG, "out is NULL");
    if (channels_org < 1 || channels_net < 1 || channels_bn < 1 || compression_level < 1)
        return fail(CAE_ERR_ARG, "bad model dimensions");
    if (kernel_size != 3 && kernel_size != 5)
        return fail(CAE_ERR_UNSUPPORTED, "kernel_size %d not supported (3 or 5)", kernel_size);
    // (the 192-channel limit of the conv kernels is enforced per layer in cae_model_set_layer;
    //  a handle that only carries entropy tables may have any number of channels)
    Model *m = new Model();
    m->c_org = channels_org;
    m->c_net = channels_net;
    m->c_bn = channels_bn;
    m->L = compression_level;
    m->ks = kernel_size;
    m->enc.resize(m->L);
    m->dec.resize(m->L);
    // no HIP call here: the host entropy coder of a handle works without a GPU; device
    // state is created on first device use (Model::ensure_device)
    *out = reinterpret_cast<cae_model_t *>(m);
    return CAE_OK;
}

void cae_model_destroy(cae_model_t *mm) {
    if (mm) {
        (void)hipDeviceSynchronize();
        delete reinterpret_cast<Model *>(mm);
    }
}

int cae_model_set_layer(cae_model_t *mm, int track, int index, int cin, int cout, const float *w, const float *bias,
                        const float *beta, const float *gamma) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !w) return fail(CAE_ERR_ARG, "NULL model or weight");
    Layer *lp;
    CAE_TRY(layer_of(m, track, index, lp));
    if ((beta == nullptr) != (gamma == nullptr)) return fail(CAE_ERR_ARG, "beta and gamma must come together");
    const int ct = round_ct(cout);
    if (ct < 0 || round_ct(cin) < 0) return fail(CAE_ERR_UNSUPPORTED, "more than 192 channels not supported");
    std::lock_guard<std::mutex> lk(m->mu);
    Layer &l = *lp;
    l.cin = cin;
    l.cout = cout;
    l.ct = ct;
    l.chunks = (cin + 7) / 8;
    l.set = true;
    CAE_TRY(l.wp.upload(pack_weights(w, track == CAE_SYNTHESIS, cin, cout, m->ks, ct)));
    CAE_TRY(upload_channels(l.bias, bias, cout, ct, 0.0f));
    // the layers with a kernel of their own: the first analysis layer, the last synthesis layer
    const bool first = track == CAE_ANALYSIS && index == 0 && cin <= 4;
    const bool last = track == CAE_SYNTHESIS && index == m->L - 1 && cout <= 4 && beta == nullptr;
    l.wp_edge.reset();
    if (first)
        CAE_TRY(l.wp_edge.upload(pack_first(w, cin, cout, m->ks, ct)));
    else if (last)
        CAE_TRY(l.wp_edge.upload(pack_last(w, cin, cout, m->ks)));
    l.f16_bad = false;
    if (m->precision == 1) {
        // the split format holds |v| <= 65504: a model with larger (or non-finite) weights runs on the fp32 kernels
        const size_t nw = (size_t)cin * cout * m->ks * m->ks;
        l.f16_bad = !fits_f16(w, nw) || (gamma && !fits_f16(gamma, (size_t)cout * cout));
        l.wp_edge16.reset();
        if (first)
            CAE_TRY(l.wp_edge16.upload(pack_first_f16(w, cin, cout, m->ks, ct)));
        else if (last)
            CAE_TRY(l.wp_edge16.upload(pack_last_f16(w, cin, cout, m->ks)));
        l.wp_pmap16.reset();
        if (last && m->ks == 3 && cout <= 3) CAE_TRY(l.wp_pmap16.upload(pack_pmap_f16(w, cin, cout, round_ct(cin))));
        CAE_TRY(l.wp16.upload(pack_weights_f16(w, track == CAE_SYNTHESIS, cin, cout, m->ks, ct)));
        if (gamma) CAE_TRY(l.gp16.upload(pack_gamma_f16(gamma, cout, ct)));
    }
    l.gdn = beta != nullptr;
    if (l.gdn) {
        CAE_TRY(upload_channels(l.beta, beta, cout, ct, 1.0f));
        CAE_TRY(l.gp.upload(pack_gamma(gamma, cout, ct)));
    }
    return CAE_OK;
}

int cae_model_set_layer_act(cae_model_t *mm, int track, int index, int act, const float *pre_w, const float *pre_b) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m) return fail(CAE_ERR_ARG, "NULL model");
    Layer *lp;
    CAE_TRY(layer_of(m, track, index, lp));
    if (act < 0 || act > 2) return fail(CAE_ERR_ARG, "bad activation %d", act);
    std::lock_guard<std::mutex> lk(m->mu);
    Layer &l = *lp;
    if (!l.set) return fail(CAE_ERR_ARG, "set the layer before its activation");
    if (l.gdn && (act != 0 || pre_w)) return fail(CAE_ERR_ARG, "a GDN unit has no other activation");
    if (pre_b && !pre_w) return fail(CAE_ERR_ARG, "pre-convolution bias without weight");
    l.act = act;
    l.stages.clear();
    if (pre_w) {
        int rc = set_stage(m, track, l, 0, pre_w, pre_b, nullptr, nullptr, act, 0, 0);
        if (rc) return rc;
    }
    return CAE_OK;
}

int cae_model_set_layer_stage(cae_model_t *mm, int track, int index, int stage, const float *w, const float *bias,
                              const float *beta, const float *gamma, int act, int add_residual, int post_act) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !w) return fail(CAE_ERR_ARG, "NULL model or weight");
    Layer *lp;
    CAE_TRY(layer_of(m, track, index, lp));
    if (stage < 0 || stage > 1) return fail(CAE_ERR_ARG, "a unit has at most two stride-1 stages");
    if (act < 0 || act > 2 || post_act < 0 || post_act > 2) return fail(CAE_ERR_ARG, "bad activation");
    if ((beta == nullptr) != (gamma == nullptr)) return fail(CAE_ERR_ARG, "beta and gamma must come together");
    if (beta && act != 0) return fail(CAE_ERR_ARG, "a GDN stage has no other activation");
    std::lock_guard<std::mutex> lk(m->mu);
    Layer &l = *lp;
    if (!l.set) return fail(CAE_ERR_ARG, "set the layer before its stages");
    if (stage > (int)l.stages.size()) return fail(CAE_ERR_ARG, "set stage 0 before stage 1");
    return set_stage(m, track, l, stage, w, bias, beta, gamma, act, add_residual, post_act);
}

int cae_model_set_color_layer(cae_model_t *mm, int index, int cin, int cout, const float *w, const float *bias) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !w) return fail(CAE_ERR_ARG, "NULL model or weight");
    if (index < 0 || index >= m->L - 1) return fail(CAE_ERR_ARG, "colour layer index %d out of range", index);
    if (cout < 1 || round_ct(cout) < 0 || round_ct(cin) < 0) return fail(CAE_ERR_UNSUPPORTED, "more than 192 channels not supported");
    std::lock_guard<std::mutex> lk(m->mu);
    Layer &l = m->dec[index];
    if (!l.set) return fail(CAE_ERR_ARG, "set the synthesis layer before its colour layer");
    if (cin != l.cout) return fail(CAE_ERR_ARG, "colour layer %d expects %d input channels, the level produces %d", index, cin, l.cout);
    const int ct = round_ct(cout);
    CAE_TRY(l.color_wp.upload(pack_weights(w, false, cin, cout, m->ks, ct)));
    CAE_TRY(upload_channels(l.color_bias, bias, cout, ct, 0.0f));
    l.color_cout = cout;
    l.color_w4.reset();
    if (cin <= 128 && cout <= 4) CAE_TRY(l.color_w4.upload(pack_color4(w, cin, cout, m->ks)));
    l.color_wp16.reset();
    if (m->precision == 1 && ct == 1) {  // f16x3: colour layers to at most 32 channels (wider: the fp32 path)
        if (!fits_f16(w, (size_t)cin * cout * m->ks * m->ks)) l.f16_bad = true;
        CAE_TRY(l.color_wp16.upload(pack_weights_f16(w, false, cin, cout, m->ks, ct)));
    }
    return CAE_OK;
}

int cae_model_set_precision(cae_model_t *mm, int precision) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m) return fail(CAE_ERR_ARG, "NULL model");
    if (precision != 0 && precision != 1) return fail(CAE_ERR_ARG, "precision must be 0 (fp32) or 1 (f16x3)");
    std::lock_guard<std::mutex> lk(m->mu);
    m->precision = precision;
    return CAE_OK;
}

int64_t cae_last_range_ticket(void) { return g_last_ticket; }

void cae_thread_force_fp32(int on) { g_force_fp32 = on != 0; }

int cae_range_check(cae_model_t *mm, int64_t ticket, int *overflowed) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !overflowed) return fail(CAE_ERR_ARG, "NULL argument");
    *overflowed = 0;
    if (ticket == 0) return CAE_OK;  // an fp32 call: nothing to check
    std::lock_guard<std::mutex> lk(m->mu);
    if (ticket < 0 || ticket > m->flag_seq || !m->flags) return fail(CAE_ERR_ARG, "unknown range ticket");
    if (m->flag_seq - ticket >= Model::kFlagSlots)
        return fail(CAE_ERR_ARG, "range ticket too old (%d calls are tracked)", Model::kFlagSlots);
    *overflowed = *(volatile int *)(m->flags + ticket % Model::kFlagSlots) != 0;
    return CAE_OK;
}

int cae_model_effective_precision(cae_model_t *mm, int *precision) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !precision) return fail(CAE_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(m->mu);
    *precision = m->f16_usable() ? 1 : 0;
    return CAE_OK;
}

int cae_model_set_entropy(cae_model_t *mm, int channels, int cdf_stride, const int32_t *cdf, const int32_t *cdf_length,
                          const int32_t *offset, const float *medians) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !cdf || !cdf_length || !offset || !medians) return fail(CAE_ERR_ARG, "NULL argument");
    if (channels != m->c_bn) return fail(CAE_ERR_ARG, "entropy model has %d channels, model %d", channels, m->c_bn);
    for (int c = 0; c < channels; ++c) {
        if (cdf_length[c] < 2 || cdf_length[c] > cdf_stride)
            return fail(CAE_ERR_ARG, "cdf_length[%d]=%d out of range", c, cdf_length[c]);
    }
    std::lock_guard<std::mutex> lk(m->mu);
    m->ent.channels = channels;
    m->ent.stride = cdf_stride;
    m->ent.cdf.assign(cdf, cdf + (size_t)channels * cdf_stride);
    m->ent.len.assign(cdf_length, cdf_length + channels);
    m->ent.off.assign(offset, offset + channels);
    m->ent.medians.assign(medians, medians + channels);
    m->ent.build_tables();
    ++m->ent_version;
    m->medians_dirty = true;
    return CAE_OK;
}

static int analysis_impl(cae_model_t *mm, const void *tiles, int fmt, int n, int h, int w, void *latents, bool symbols,
                         float *const *levels, void *stream);

int cae_analysis(cae_model_t *mm, const void *tiles, int fmt, int n, int h, int w, float *latents, void *stream) {
    return analysis_impl(mm, tiles, fmt, n, h, w, latents, false, nullptr, stream);
}

int cae_analysis_levels(cae_model_t *mm, const void *tiles, int fmt, int n, int h, int w, float *latents,
                        float *const *levels, void *stream) {
    return analysis_impl(mm, tiles, fmt, n, h, w, latents, false, levels, stream);
}

int cae_analysis_symbols(cae_model_t *mm, const void *tiles, int fmt, int n, int h, int w, int32_t *symbols,
                         void *stream) {
    return analysis_impl(mm, tiles, fmt, n, h, w, symbols, true, nullptr, stream);
}

// Every reflect-padded convolution of the analysis track (strided layers and stride-1 stages; F.pad(mode='reflect')
// needs pad < size, as the reference) sees an input above the padding k//2?  Level i's input is h x w halved i times.
static int check_reflect_levels(const Model *m, int h, int w) {
    const int P = m->ks / 2;
    for (int i = 0; i < m->L; ++i, h = (h + 1) / 2, w = (w + 1) / 2)
        if (h <= P || w <= P)
            return fail(CAE_ERR_ARG, "analysis level %d input %d x %d too small for reflect padding %d", i, h, w, P);
    return CAE_OK;
}

static int analysis_impl(cae_model_t *mm, const void *tiles, int fmt, int n, int h, int w, void *latents, bool symbols,
                         float *const *levels, void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !tiles || !latents) return fail(CAE_ERR_ARG, "NULL argument");
    if (symbols && m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if (n < 1 || h < 2 || w < 2) return fail(CAE_ERR_ARG, "bad tile batch %dx%dx%d", n, h, w);
    if (fmt != CAE_FMT_U8_HWC && fmt != CAE_FMT_F32_NCHW) return fail(CAE_ERR_ARG, "bad pixel format %d", fmt);
    for (auto &l : m->enc)
        if (!l.set) return fail(CAE_ERR_ARG, "analysis layer not set");
    int rc;
    if ((rc = check_reflect_levels(m, h, w))) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(m->mu);
    if ((rc = m->ensure_device()) || (rc = m->order_stream(stream))) return rc;
    const bool f16 = m->f16_usable();
    const bool first_fused = f16 ? (bool)m->enc[0].wp_edge16 : (bool)m->enc[0].wp_edge;
    int64_t ticket = 0;
    g_last_ticket = 0;
    int *flag = f16 ? m->next_flag(&ticket) : m->flags_dev;  // (fp32 kernels never write it)

    // workspace: ws[0] = converted input, ws[1]/ws[2] ping-pong.  fp32 C8 and split C8S records are
    // both 32 B per (plane, pixel), so the same buffers serve either precision.
    const int p0 = f16 ? 2 * ((m->c_org + 15) / 16) : (m->c_org + 7) / 8;
    // f16x3: rows are padded to whole 32-pixel groups (C8S, cae_kernels_f16.hpp)
    auto row_bytes = [&](int cw) { return f16 ? c8s_row_bytes<false>(cw) : (size_t)cw * 32; };
    size_t in_bytes = first_fused ? 0 : (size_t)n * p0 * h * row_bytes(w);
    size_t maxact = 0;
    {
        int ch = h, cw = w;
        for (int i = 0; i < m->L; ++i) {
            if (!m->enc[i].stages.empty())  // stride-1 stages: same size, cin channels
                maxact = std::max(maxact, (size_t)n * round_ct(m->enc[i].cin) * 4 * ch * row_bytes(cw));
            ch = (ch + 1) / 2;
            cw = (cw + 1) / 2;
            if (i + 1 < m->L) maxact = std::max(maxact, (size_t)n * m->enc[i].ct * 4 * ch * row_bytes(cw));
        }
    }
    const bool u8_wide = f16 && !first_fused && fmt == CAE_FMT_U8_HWC;  // staged through fp32 C8 in ws[1]
    if (u8_wide) maxact = std::max(maxact, (size_t)n * p0 * h * w * 32);
    bool need_third_slot = false;  // two-stage residual units keep the unit input alive across both stages
    for (auto &l : m->enc)
        need_third_slot |= l.stages.size() > 1 || (f16 && (!conv_f16_fits(m->ks, l.ct, l.gdn) || stages_need_fp32(l)));
    if ((rc = m->ensure_ws(0, in_bytes))) return rc;
    if (maxact && ((rc = m->ensure_ws(1, maxact)) || (rc = m->ensure_ws(2, maxact)))) return rc;
    if (maxact && need_third_slot && (rc = m->ensure_ws(3, maxact))) return rc;

    ProfScope prof(m, CAE_ANALYSIS, st);
    prof.begin();
    if (!first_fused) {
        const size_t tot = (size_t)n * p0 * h * w;
        if (f16) {
            if (fmt == CAE_FMT_U8_HWC) {
                // rare (more than 4 input channels): uint8 -> fp32 C8 (exact /255) in ws[1] -> split rows in ws[0]
                hipLaunchKernelGGL(u8hwc_to_c8_kernel, dim3(ew_grid(tot)), dim3(256), 0, st, (const uint8_t *)tiles,
                                   (float *)m->ws[1].p, n, h, w, m->c_org, p0);
                hipLaunchKernelGGL(c8_to_c8s_kernel<false>, dim3(ew_grid(tot)), dim3(256), 0, st, (const float *)m->ws[1].p,
                                   (char *)m->ws[0].p, (size_t)n * p0 * h, w, flag);
            } else {
                hipLaunchKernelGGL(nchw_to_c8s_kernel<false>, dim3(ew_grid(tot)), dim3(256), 0, st,
                                   (const float *)tiles, (char *)m->ws[0].p, n, m->c_org, h, w, p0, flag);
            }
        } else if (fmt == CAE_FMT_U8_HWC) {
            hipLaunchKernelGGL(u8hwc_to_c8_kernel, dim3(ew_grid(tot)), dim3(256), 0, st, (const uint8_t *)tiles,
                               (float *)m->ws[0].p, n, h, w, m->c_org, p0);
        } else {
            hipLaunchKernelGGL(nchw_to_c8_kernel, dim3(ew_grid(tot)), dim3(256), 0, st, (const float *)tiles,
                               (float *)m->ws[0].p, n, m->c_org, h * w, p0);
        }
        HIP_TRY(hipGetLastError());
    }
    prof.end();

    const float *cur = (const float *)m->ws[0].p;
    int cur_planes = p0, ch = h, cw = w;
    int cur_idx = 0;  // workspace slot holding `cur` (0 = converted input; 1..3 rotate)
    for (int i = 0; i < m->L; ++i) {
        const Layer &l = m->enc[i];
        const bool last = i == m->L - 1;
        if (!l.stages.empty() && (rc = run_stages(m, l, false, n, ch, cw, cur, cur_idx, cur_planes, st, f16, flag))) return rc;
        const int out_idx = pick_slot(cur_idx, cur_idx);
        LayerArgs a = layer_args(m, cur, cur_planes, last ? latents : m->ws[out_idx].p, n, ch, cw, (ch + 1) / 2, (cw + 1) / 2,
                                 l.ct, l.cout, last ? (symbols ? OUT_SYM : OUT_NCHW) : OUT_C8, l.act, flag);
        a.wp = l.wp.get<float>();
        a.bias = l.bias.get<float>();
        a.gp = l.gp.get<float>();
        a.beta = l.beta.get<float>();
        if (last && symbols) a.medians = m->medians_dev.get<float>();
        prof.begin();
        if (i == 0 && first_fused) {
            FirstArgs f{tiles, fmt == CAE_FMT_U8_HWC ? 1 : 0, l.cin};
            if (f16) {
                a.wp = l.wp_edge16.get<float>();
                a.gp = l.gp16.get<float>();
                if ((rc = launch_first_f16(m->ks, l.ct, l.gdn, a, f, st))) return rc;
            } else {
                a.wp = l.wp_edge.get<float>();
                if ((rc = launch_first(m->ks, l.ct, l.gdn, a, f, st))) return rc;
            }
        } else if (f16 && conv_f16_fits(m->ks, l.ct, l.gdn) && !(l.gdn && l.ct > 4 && last)) {
            a.wp = l.wp16.get<float>();
            a.gp = l.gp16.get<float>();
            if ((rc = launch_conv_f16(m->ks, l.ct, l.gdn, l.cin, a, st))) return rc;
        } else if (f16) {
            // this layer on the exact-fp32 kernel: split rows -> fp32 C8, convolution, (fp32 C8 -> split rows)
            const int tmp_in = pick_slot(cur_idx, out_idx);
            const size_t rows = (size_t)n * cur_planes * ch;
            hipLaunchKernelGGL(c8s_to_c8_kernel<false>, dim3(ew_grid(rows * cw)), dim3(256), 0, st, (const char *)cur,
                               (float *)m->ws[tmp_in].p, rows, cw);
            HIP_TRY(hipGetLastError());
            a.in = (const float *)m->ws[tmp_in].p;
            void *final_out = a.out;
            if (!last) a.out = m->ws[cur_idx == 0 ? pick_slot(tmp_in, out_idx) : cur_idx].p;  // the input slot is free now
            if ((rc = launch_conv(m->ks, l.ct, l.gdn, l.cin, a, st))) return rc;
            if (!last) {
                const size_t orows = (size_t)n * l.ct * 4 * a.OH;
                hipLaunchKernelGGL(c8_to_c8s_kernel<false>, dim3(ew_grid(orows * a.OW)), dim3(256), 0, st, (const float *)a.out,
                                   (char *)final_out, orows, a.OW, flag);
                HIP_TRY(hipGetLastError());
                a.out = final_out;
            }
        } else {
            if ((rc = launch_conv(m->ks, l.ct, l.gdn, l.cin, a, st))) return rc;
        }
        prof.end();
        if (!last && levels && levels[i]) {  // the unit's output as the next unit reads it (split: exactly hi + lo)
            const size_t t2 = (size_t)n * l.cout * a.OH * a.OW;
            if (f16)
                hipLaunchKernelGGL(c8s_to_nchw_kernel<false>, dim3(ew_grid(t2)), dim3(256), 0, st, (const char *)a.out,
                                   levels[i], n, l.cout, a.OH, a.OW, l.ct * 4);
            else
                hipLaunchKernelGGL(c8_to_nchw_kernel, dim3(ew_grid(t2)), dim3(256), 0, st, (const float *)a.out,
                                   levels[i], n, l.cout, a.OH * a.OW, l.ct * 4);
            HIP_TRY(hipGetLastError());
        }
        cur = (const float *)a.out;
        cur_planes = l.ct * 4;
        ch = a.OH;
        cw = a.OW;
        cur_idx = out_idx;
    }
    return CAE_OK;
}

static int synthesis_impl(cae_model_t *mm, const float *latents, const int32_t *symbols, int n, int lh, int lw, void *out,
                          int fmt, float *const *bridges, float *const *colors, void *stream, int scale = 0);

int cae_synthesis(cae_model_t *mm, const float *latents, int n, int lh, int lw, void *out, int fmt,
                  float *const *bridges, void *stream) {
    if (!latents) return fail(CAE_ERR_ARG, "NULL argument");
    return synthesis_impl(mm, latents, nullptr, n, lh, lw, out, fmt, bridges, nullptr, stream);
}

int cae_synthesis_multiscale(cae_model_t *mm, const float *latents, int n, int lh, int lw, void *out, int fmt,
                             float *const *bridges, float *const *colors, void *stream) {
    if (!latents) return fail(CAE_ERR_ARG, "NULL argument");
    return synthesis_impl(mm, latents, nullptr, n, lh, lw, out, fmt, bridges, colors, stream);
}

int cae_synthesis_symbols(cae_model_t *mm, const int32_t *symbols, int n, int lh, int lw, void *out, int fmt,
                          void *stream) {
    if (!symbols) return fail(CAE_ERR_ARG, "NULL argument");
    return synthesis_impl(mm, nullptr, symbols, n, lh, lw, out, fmt, nullptr, nullptr, stream);
}

// Synthesis that stops at a level: units 0 .. L-1-scale, then colour layer L-1-scale into `out` (the image at 1 / 2^scale
// of the resolution).  scale == 0 is cae_synthesis / cae_synthesis_symbols.
static int check_scale(cae_model_t *mm, int scale) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m) return fail(CAE_ERR_ARG, "NULL argument");
    if (scale < 0 || scale >= m->L) return fail(CAE_ERR_ARG, "scale %d outside 0..%d", scale, m->L - 1);
    return CAE_OK;
}

int cae_synthesis_scale(cae_model_t *mm, const float *latents, int n, int lh, int lw, int scale, void *out, int fmt,
                        void *stream) {
    if (!latents) return fail(CAE_ERR_ARG, "NULL argument");
    CAE_TRY(check_scale(mm, scale));
    return synthesis_impl(mm, latents, nullptr, n, lh, lw, out, fmt, nullptr, nullptr, stream, scale);
}

int cae_synthesis_symbols_scale(cae_model_t *mm, const int32_t *symbols, int n, int lh, int lw, int scale, void *out,
                                int fmt, void *stream) {
    if (!symbols) return fail(CAE_ERR_ARG, "NULL argument");
    CAE_TRY(check_scale(mm, scale));
    return synthesis_impl(mm, nullptr, symbols, n, lh, lw, out, fmt, nullptr, nullptr, stream, scale);
}

static int synthesis_impl(cae_model_t *mm, const float *latents, const int32_t *symbols, int n, int lh, int lw, void *out,
                          int fmt, float *const *bridges, float *const *colors, void *stream, int scale) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !out) return fail(CAE_ERR_ARG, "NULL argument");
    // scale > 0 (cae_synthesis_scale): the track stops after unit `stop`, whose colour layer writes `out`
    const int stop = m->L - 1 - scale, nrun = stop + 1;
    if (symbols && m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if (n < 1 || lh < 1 || lw < 1) return fail(CAE_ERR_ARG, "bad latent batch %dx%dx%d", n, lh, lw);
    if (fmt != CAE_FMT_U8_HWC && fmt != CAE_FMT_F32_NCHW) return fail(CAE_ERR_ARG, "bad pixel format %d", fmt);
    for (auto &l : m->dec)
        if (!l.set) return fail(CAE_ERR_ARG, "synthesis layer not set");
    // colour layers are reflect-padded stride-1 convolutions on level i's output (lh, lw doubled i + 1 times)
    for (int i = 0; colors && i + 1 < m->L; ++i)
        if (colors[i] && ((lh << (i + 1)) <= m->ks / 2 || (lw << (i + 1)) <= m->ks / 2))
            return fail(CAE_ERR_ARG, "colour layer %d input %d x %d too small for reflect padding %d", i, lh << (i + 1),
                        lw << (i + 1), m->ks / 2);
    if (scale > 0) {
        const Layer &l = m->dec[stop];
        if (!l.color_wp) return fail(CAE_ERR_ARG, "colour layer %d not set", stop);
        if ((lh << nrun) <= m->ks / 2 || (lw << nrun) <= m->ks / 2)
            return fail(CAE_ERR_ARG, "colour layer %d input %d x %d too small for reflect padding %d", stop, lh << nrun,
                        lw << nrun, m->ks / 2);
    }
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(m->mu);
    int rc;
    if ((rc = m->ensure_device()) || (rc = m->order_stream(stream))) return rc;
    const bool f16 = m->f16_usable();
    if (scale > 0 && f16 && !m->dec[stop].color_w4 && !m->dec[stop].color_wp16)
        return fail(CAE_ERR_UNSUPPORTED, "f16x3: colour layers to more than 32 channels run on the fp32 path: set precision 0");
    int64_t ticket = 0;
    g_last_ticket = 0;
    int *flag = f16 ? m->next_flag(&ticket) : m->flags_dev;

    // planes of the converted latents: padded so whole MFMA k-steps can be read (zero channels)
    // (fp32: an EVEN number of 8-channel planes -- the last-layer kernel consumes 16-channel groups, and with one layer it
    //  reads these planes directly: 72 latent channels = 9 planes made it read a tenth one past the buffer)
    const int p0 = f16 ? 4 * ((m->c_bn + 31) / 32) : 2 * ((m->c_bn + 15) / 16);
    // f16x3: the synthesis track keeps its activations in C8SP rows (pitch = whole 64-pixel blocks)
    auto row_bytes = [&](int cw) { return f16 ? c8s_row_bytes<true>(cw) : (size_t)cw * 32; };
    size_t in_bytes = (size_t)n * p0 * lh * row_bytes(lw);
    size_t maxact = 0;
    {
        int ch = lh, cw = lw;
        for (int i = 0; i < nrun; ++i) {  // (the levels that run)
            if (!m->dec[i].stages.empty())
                maxact = std::max(maxact, (size_t)n * round_ct(m->dec[i].cin) * 4 * ch * row_bytes(cw));
            ch *= 2;
            cw *= 2;
            if (i + 1 < m->L) maxact = std::max(maxact, (size_t)n * m->dec[i].ct * 4 * ch * row_bytes(cw));
        }
    }
    bool need_third_slot = false;
    for (int i = 0; i < nrun; ++i)
        need_third_slot |= m->dec[i].stages.size() > 1 || (f16 && stages_need_fp32(m->dec[i]));
    if (scale > 0 && !m->dec[stop].color_w4 && fmt == CAE_FMT_U8_HWC) {
        // generic colour launch: fp32 NCHW into a spare slot, then the uint8 conversion
        maxact = std::max(maxact, (size_t)n * m->dec[stop].color_cout * (lh << nrun) * (lw << nrun) * sizeof(float));
    }
    if ((rc = m->ensure_ws(0, in_bytes))) return rc;
    if (maxact && ((rc = m->ensure_ws(1, maxact)) || (rc = m->ensure_ws(2, maxact)))) return rc;
    if (maxact && need_third_slot && (rc = m->ensure_ws(3, maxact))) return rc;

    ProfScope prof(m, CAE_SYNTHESIS, st);
    prof.begin();
    const size_t tot = (size_t)n * p0 * lh * lw;
    if (f16)
        hipLaunchKernelGGL(nchw_to_c8s_kernel<true>, dim3(ew_grid(tot)), dim3(256), 0, st, latents, (char *)m->ws[0].p, n,
                           m->c_bn, lh, lw, p0, flag, symbols, m->medians_dev.get<float>());
    else
        hipLaunchKernelGGL(nchw_to_c8_kernel, dim3(ew_grid(tot)), dim3(256), 0, st, latents, (float *)m->ws[0].p, n,
                           m->c_bn, lh * lw, p0, symbols, m->medians_dev.get<float>());
    HIP_TRY(hipGetLastError());
    prof.end();

    // Product-map form of the last two layers (cae_kernels_f16.hpp, pmap): layer L-2 stores the products of its output
    // with the last layer's weights, the last layer is a gather.  Needs the f16x3 transposed-convolution kernel for
    // layer L-2, k = 3, at most 3 image channels, and nobody asking for layer L-2's own output (bridges / colours).
    bool use_pmap = false;
    if (f16 && scale == 0 && m->L >= 2 && m->ks == 3 && getenv("CAE_NO_PMAP") == nullptr) {
        const Layer &lp = m->dec[m->L - 2], &ll = m->dec[m->L - 1];
        // (conv_f16-style LDS budget: two 33-KiB stages + the transpose buffers fit for k = 3 and up to 128 channels)
        use_pmap = ll.wp_pmap16 && !ll.gdn && ll.stages.empty() && lp.stages.empty() && lp.ct <= 4 && lp.cout == ll.cin &&
                   !(bridges && bridges[m->L - 2]) && !(colors && colors[m->L - 2]);
    }
    if (use_pmap) maxact = std::max(maxact, (size_t)n * (lh << (m->L - 1)) * (lw << (m->L - 1)) * 128);
    if (use_pmap && ((rc = m->ensure_ws(1, maxact)) || (rc = m->ensure_ws(2, maxact)))) return rc;

    const float *cur = (const float *)m->ws[0].p;
    int cur_planes = p0, ch = lh, cw = lw;
    int cur_idx = 0;
    for (int i = 0; i < nrun; ++i) {
        const Layer &l = m->dec[i];
        const bool last = i == m->L - 1;
        if (use_pmap && last) {  // the gather half of the product map
            prof.begin();
            const int gtx = (cw + 15) / 16, gty = (ch + 15) / 16;
            hipLaunchKernelGGL(pmap_gather_kernel, dim3((unsigned)((size_t)n * gtx * gty)), dim3(256), 0, st, cur,
                               l.bias.get<float>(), out, n, ch, cw, l.cout, fmt == CAE_FMT_U8_HWC ? OUT_U8HWC : OUT_NCHW, gtx,
                               gty);
            HIP_TRY(hipGetLastError());
            prof.end();
            break;
        }
        if (!l.stages.empty() && (rc = run_stages(m, l, true, n, ch, cw, cur, cur_idx, cur_planes, st, f16, flag))) return rc;
        const int out_idx = pick_slot(cur_idx, cur_idx);
        LayerArgs a = layer_args(m, cur, cur_planes, last ? out : m->ws[out_idx].p, n, ch, cw, 2 * ch, 2 * cw, l.ct, l.cout,
                                 last ? (fmt == CAE_FMT_U8_HWC ? OUT_U8HWC : OUT_NCHW) : OUT_C8, l.act, flag);
        a.wp = l.wp.get<float>();
        a.bias = l.bias.get<float>();
        a.gp = l.gp.get<float>();
        a.beta = l.beta.get<float>();
        if (use_pmap && i == m->L - 2) {
            a.outfmt = OUT_PMAP;
            a.pm = m->dec[m->L - 1].wp_pmap16.p;
        }
        prof.begin();
        if (f16) {
            a.gp = l.gp16.get<float>();
            if (last && l.wp_edge16 && last_f16_fits(m->ks, l.cin)) {
                a.wp = l.wp_edge16.get<float>();
                if ((rc = launch_last_f16(m->ks, l.cin, a, st))) return rc;
            } else {
                if (l.act && l.ct > 4)  // (the 192-channel transposed-convolution kernel carries no activation: registers)
                    return fail(CAE_ERR_UNSUPPORTED, "f16x3: LeakyReLU / ReLU synthesis layers wider than 128 channels run "
                                                     "on the fp32 path: set precision 0");
                a.wp = l.wp16.get<float>();
                if ((rc = launch_deconv_f16(m->ks, l.ct, l.gdn, l.cin, a, st))) return rc;
            }
        } else if (last && l.wp_edge) {
            a.wp = l.wp_edge.get<float>();
            if ((rc = launch_last(m->ks, l.cin, a, st))) return rc;
        } else {
            if ((rc = launch_deconv(m->ks, l.ct, l.gdn, l.cin, a, st))) return rc;
        }
        prof.end();
        if (!last && colors && colors[i]) {  // colour layer of this level (_autoencoders.py:417-436, :448-449)
            if (!l.color_wp) return fail(CAE_ERR_ARG, "colour layer %d not set", i);
            if (f16 && !l.color_wp16)
                return fail(CAE_ERR_UNSUPPORTED, "f16x3: colour layers to more than 32 channels run on the fp32 path: set precision 0");
            if ((rc = launch_color(m, l, f16, (const float *)a.out, l.ct * 4, n, a.OH, a.OW, colors[i], flag, st))) return rc;
        }
        if (!last && bridges && bridges[i]) {
            const size_t t2 = (size_t)n * l.cout * a.OH * a.OW;
            if (f16)
                hipLaunchKernelGGL(c8s_to_nchw_kernel<true>, dim3(ew_grid(t2)), dim3(256), 0, st, (const char *)a.out,
                                   bridges[i], n, l.cout, a.OH, a.OW, l.ct * 4);
            else
                hipLaunchKernelGGL(c8_to_nchw_kernel, dim3(ew_grid(t2)), dim3(256), 0, st, (const float *)a.out,
                                   bridges[i], n, l.cout, a.OH * a.OW, l.ct * 4);
            HIP_TRY(hipGetLastError());
        }
        cur = (const float *)a.out;
        cur_planes = l.ct * 4;
        ch = a.OH;
        cw = a.OW;
        cur_idx = out_idx;
    }
    if (scale > 0) {  // colour layer of level `stop` on its activations `cur` (ch x cw), into `out`
        const Layer &l = m->dec[stop];
        const int ofmt = fmt == CAE_FMT_U8_HWC ? OUT_U8HWC : OUT_NCHW;
        prof.begin();
        if (l.color_w4) {
            if ((rc = launch_color_small(m->ks, f16, cur, cur_planes, l.cout, l.color_w4.get<float>(),
                                         l.color_bias.get<float>(), n, ch, cw, l.color_cout, out, ofmt, flag, st)))
                return rc;
        } else {
            // more than 128 input or 4 image channels: the generic stride-1 launch (fp32 NCHW), + the uint8 conversion
            float *img = ofmt == OUT_NCHW ? (float *)out : (float *)m->ws[pick_slot(cur_idx, cur_idx)].p;
            if ((rc = launch_color(m, l, f16, cur, cur_planes, n, ch, cw, img, flag, st))) return rc;
            if (ofmt == OUT_U8HWC && (rc = launch_nchw_to_u8hwc(img, out, n, l.color_cout, (size_t)ch * cw, st))) return rc;
        }
        prof.end();
    }
    return CAE_OK;
}

int cae_gdn_forward(cae_model_t *mm, int track, int index, const float *x, int n, int h, int w, float *y, void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !x || !y) return fail(CAE_ERR_ARG, "NULL argument");
    Layer *lp;
    CAE_TRY(layer_of(m, track, index, lp));
    if (n < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad tensor shape");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(m->mu);
    const Layer &l = *lp;
    if (!l.set || !l.gdn) return fail(CAE_ERR_ARG, "layer has no GDN");
    const int planes = l.ct * 4;
    int rc;
    if ((rc = m->ensure_device()) || (rc = m->order_stream(stream))) return rc;
    if ((rc = m->ensure_ws(0, (size_t)n * planes * h * w * 32))) return rc;
    const size_t tot = (size_t)n * planes * h * w;
    hipLaunchKernelGGL(nchw_to_c8_kernel, dim3(ew_grid(tot)), dim3(256), 0, st, x, (float *)m->ws[0].p, n, l.cout, h * w,
                       planes);
    HIP_TRY(hipGetLastError());
    LayerArgs a = layer_args(m, (const float *)m->ws[0].p, planes, y, n, h, w, h, w, l.ct, l.cout, OUT_NCHW, 0, nullptr);
    a.gp = l.gp.get<float>();
    a.beta = l.beta.get<float>();
    return launch_gdn(l.ct, track == CAE_SYNTHESIS, a, st);
}

int cae_tile_sse(const uint8_t *a, const uint8_t *b, int n, size_t elems, double *sse, void *stream) {
    if (!a || !b || !sse) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || n > 65535 || elems < 1) return fail(CAE_ERR_ARG, "bad shape");  // n is the grid's y dimension
    hipStream_t st = (hipStream_t)stream;
    // the float64 output doubles as the exact integer accumulator (same 8-byte cells)
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(sse);
    HIP_TRY(hipMemsetAsync(acc, 0, (size_t)n * 8, st));
    const unsigned bx = (unsigned)std::min<size_t>(std::max<size_t>(elems / 16 / 256, 1), 64);  // (byte loop: same grid)
    hipLaunchKernelGGL(tile_sse_kernel, dim3(bx, n), dim3(256), 0, st, a, b, elems, acc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(u64_to_f64_kernel, dim3((n + 255) / 256), dim3(256), 0, st, acc, sse, n);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_tile_ssim(const uint8_t *a, const uint8_t *b, int n, int h, int w, int c, double *ssim, double *workspace,
                  size_t workspace_elems, void *stream) {
    if (!a || !b || !ssim || !workspace) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || n > 65535 || c < 1) return fail(CAE_ERR_ARG, "bad shape");
    if (h < 7 || w < 7) return fail(CAE_ERR_ARG, "tiles must be at least 7x7 (the SSIM window)");
    const int oh = h - 6, ow = w - 6;
    const int bxr = (ow + 31) / 32, bpt = bxr * ((oh + 31) / 32);
    if (workspace_elems < (size_t)n * bpt)
        return fail(CAE_ERR_ARG, "workspace too small: %zu doubles needed", (size_t)n * bpt);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tile_ssim_kernel, dim3(bpt, n), dim3(256), 0, st, a, b, h, w, c, bxr, bpt, workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(n), dim3(256), 0, st, workspace, bpt, (double)oh * ow * c, ssim);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_tile_delta_e(const uint8_t *a, const uint8_t *b, int n, size_t pixels, double *delta, double *workspace,
                     size_t workspace_elems, void *stream) {
    if (!a || !b || !delta || !workspace) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || n > 65535 || pixels < 1) return fail(CAE_ERR_ARG, "bad shape");
    const int bpt = (int)std::min<size_t>((pixels + 255) / 256, 128);
    if (workspace_elems < (size_t)n * bpt)
        return fail(CAE_ERR_ARG, "workspace too small: %zu doubles needed", (size_t)n * bpt);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tile_delta_e_kernel, dim3(bpt, n), dim3(256), 0, st, a, b, pixels, bpt, workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(n), dim3(256), 0, st, workspace, bpt, (double)pixels, delta);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_u8hwc_to_planes(const uint8_t *tiles, int n, int h, int w, int c, float *planes, void *stream) {
    if (!tiles || !planes) return fail(CAE_ERR_ARG, "NULL argument");
    if (n < 1 || h < 1 || w < 1 || c < 1) return fail(CAE_ERR_ARG, "bad shape");
    hipLaunchKernelGGL(u8hwc_to_planes_kernel, dim3(ew_grid((size_t)n * c * h * w)), dim3(256), 0, (hipStream_t)stream,
                       tiles, planes, n, h, w, c);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_avgpool2(const float *in, int planes, int h, int w, float *out, void *stream) {
    if (!in || !out) return fail(CAE_ERR_ARG, "NULL argument");
    if (planes < 1 || h < 1 || w < 1) return fail(CAE_ERR_ARG, "bad shape");
    const int oh = (h + 2 * (h & 1) - 2) / 2 + 1, ow = (w + 2 * (w & 1) - 2) / 2 + 1;
    hipLaunchKernelGGL(avgpool2_kernel, dim3(ew_grid((size_t)planes * oh * ow)), dim3(256), 0, (hipStream_t)stream, in,
                       out, planes, h, w, oh, ow);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_msssim_level(const float *x, const float *y, int planes, int h, int w, const float *window11, double *ssim_cs,
                     double *workspace, size_t workspace_elems, void *stream) {
    if (!x || !y || !window11 || !ssim_cs || !workspace) return fail(CAE_ERR_ARG, "NULL argument");
    if (planes < 1 || planes > 65535) return fail(CAE_ERR_ARG, "bad plane count");
    if (h < 11 || w < 11) return fail(CAE_ERR_ARG, "image smaller than the 11-tap window");
    const int oh = h - 10, ow = w - 10;
    const int bxr = (ow + 31) / 32, bpp = bxr * ((oh + 31) / 32);
    if (workspace_elems < (size_t)planes * bpp * 2)
        return fail(CAE_ERR_ARG, "workspace too small: %zu doubles needed", (size_t)planes * bpp * 2);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(msssim_level_kernel, dim3(bpp, planes), dim3(256), 0, st, x, y, h, w, bxr, bpp, window11, workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(msssim_reduce_kernel, dim3(planes), dim3(256), 0, st, workspace, bpp, (double)oh * ow, ssim_cs);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_model_set_profiling(cae_model_t *mm, int enable) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m) return fail(CAE_ERR_ARG, "NULL model");
    std::lock_guard<std::mutex> lk(m->mu);
    m->profiling = enable != 0;
    return CAE_OK;
}

int cae_model_get_profile(cae_model_t *mm, int track, double *ms, int n_slots, int *calls, int reset) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !ms || n_slots < 1) return fail(CAE_ERR_ARG, "NULL argument");
    if (track != CAE_ANALYSIS && track != CAE_SYNTHESIS) return fail(CAE_ERR_ARG, "bad track %d", track);
    std::lock_guard<std::mutex> lk(m->mu);
    for (int i = 0; i < n_slots; ++i) ms[i] = 0.0;
    auto &calls_v = m->prof[track];
    for (auto &call : calls_v)
        for (size_t i = 0; i < call.size(); ++i) {
            HIP_TRY(hipEventSynchronize((hipEvent_t)call[i].second));
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, (hipEvent_t)call[i].first, (hipEvent_t)call[i].second));
            if ((int)i < n_slots) ms[i] += t;
        }
    if (calls) *calls = (int)calls_v.size();
    if (reset) {
        for (auto &call : calls_v)
            for (auto &e : call) {
                (void)hipEventDestroy((hipEvent_t)e.first);
                (void)hipEventDestroy((hipEvent_t)e.second);
            }
        calls_v.clear();
    }
    return CAE_OK;
}

int cae_quantize(cae_model_t *mm, const float *latents, int n, int hw, int32_t *symbols, void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !latents || !symbols) return fail(CAE_ERR_ARG, "NULL argument");
    if (m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if (n < 1 || hw < 1) return fail(CAE_ERR_ARG, "bad shape");
    {
        std::lock_guard<std::mutex> lk(m->mu);
        int rc = m->ensure_device();
        if (rc) return rc;
    }
    const size_t total = (size_t)n * m->c_bn * hw;
    hipLaunchKernelGGL(quantize_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, latents,
                       m->medians_dev.get<float>(), symbols, m->c_bn, hw, total);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_model_set_density(cae_model_t *mm, int channels, int n_filters, const int *filters, const float *const *matrices,
                          const float *const *biases, const float *const *factors, float likelihood_bound) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !filters || !matrices || !biases || !factors) return fail(CAE_ERR_ARG, "NULL argument");
    if (channels != m->c_bn) return fail(CAE_ERR_ARG, "density model has %d channels, model %d", channels, m->c_bn);
    if (n_filters < 1) return fail(CAE_ERR_UNSUPPORTED, "density network needs at least one hidden layer");
    int R = 0;
    for (int i = 0; i < n_filters; ++i) {
        if (filters[i] < 1) return fail(CAE_ERR_ARG, "filters[%d]=%d", i, filters[i]);
        R = std::max(R, filters[i]);
    }
    if (R > 8) return fail(CAE_ERR_UNSUPPORTED, "density filters wider than 8 are not supported (got %d)", R);
    for (int i = 0; i <= n_filters; ++i)
        if (!matrices[i] || !biases[i] || (i < n_filters && !factors[i])) return fail(CAE_ERR_ARG, "NULL parameter %d", i);
    const int K = n_filters;
    const int per = 3 * R + (K - 1) * (R * R + 2 * R) + R + 1;
    std::vector<float> packed((size_t)channels * per, 0.f);
    // narrower layers are embedded in width R with zero weights: the extra units stay exactly 0
    auto width = [&](int i) { return i == 0 ? 1 : (i == K + 1 ? 1 : filters[i - 1]); };  // F[i]
    for (int c = 0; c < channels; ++c) {
        float *o = packed.data() + (size_t)c * per;
        for (int i = 0; i <= K; ++i) {
            const int fin = width(i), fout = width(i + 1);
            const float *M = matrices[i] + (size_t)c * fout * fin;
            const float *b = biases[i] + (size_t)c * fout;
            const float *t = i < K ? factors[i] + (size_t)c * fout : nullptr;
            if (i == 0) {
                for (int j = 0; j < fout; ++j) { o[j] = M[j]; o[R + j] = b[j]; o[2 * R + j] = t[j]; }
                o += 3 * R;
            } else if (i < K) {
                for (int j = 0; j < fout; ++j) {
                    for (int k = 0; k < fin; ++k) o[j * R + k] = M[j * fin + k];
                    o[R * R + j] = b[j];
                    o[R * R + R + j] = t[j];
                }
                o += R * R + 2 * R;
            } else {
                for (int k = 0; k < fin; ++k) o[k] = M[k];
                o[R] = b[0];
            }
        }
    }
    std::lock_guard<std::mutex> lk(m->mu);
    m->density.swap(packed);
    m->density_r = R;
    m->density_k = K;
    m->density_per_channel = per;
    m->density_bound = likelihood_bound > 0.f ? likelihood_bound : 0.f;
    m->density_dirty = true;
    return CAE_OK;
}

int cae_model_set_likelihood_form(cae_model_t *mm, int form) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m) return fail(CAE_ERR_ARG, "NULL model");
    if (form != 0 && form != 1) return fail(CAE_ERR_ARG, "likelihood form must be 0 (plain) or 1 (sign trick)");
    std::lock_guard<std::mutex> lk(m->mu);
    m->likelihood_plain = form == 0;
    return CAE_OK;
}

int cae_likelihood(cae_model_t *mm, const float *latents, int n, int hw, float *y_hat, float *likelihood, double *bits,
                   void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !latents) return fail(CAE_ERR_ARG, "NULL argument");
    if (!y_hat && !likelihood && !bits) return fail(CAE_ERR_ARG, "no output requested");
    if (m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if (m->density.empty()) return fail(CAE_ERR_ARG, "density model not set");
    if (n < 1 || hw < 1 || n > 65535) return fail(CAE_ERR_ARG, "bad shape");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(m->mu);
    int rc = m->ensure_device();
    if (rc) return rc;
    double *part = nullptr;
    if (bits) {
        const size_t need = (size_t)n * m->c_bn * sizeof(double);
        if (m->bits_ws.bytes < need) {
            if (m->bits_ws) {
                HIP_TRY(hipDeviceSynchronize());
                m->bits_ws.reset();
            }
            CAE_TRY(m->bits_ws.alloc(need));
        }
        part = m->bits_ws.get<double>();
    }
    switch (m->density_r) {
        case 1: launch_likelihood<1>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        case 2: launch_likelihood<2>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        case 3: launch_likelihood<3>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        case 4: launch_likelihood<4>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        case 5: launch_likelihood<5>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        case 6: launch_likelihood<6>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        case 7: launch_likelihood<7>(m, latents, n, hw, y_hat, likelihood, part, st); break;
        default: launch_likelihood<8>(m, latents, n, hw, y_hat, likelihood, part, st); break;
    }
    HIP_TRY(hipGetLastError());
    if (bits) {
        hipLaunchKernelGGL(bits_reduce_kernel, dim3(n), dim3(256), 0, st, part, m->c_bn, bits);
        HIP_TRY(hipGetLastError());
    }
    return CAE_OK;
}

int cae_quantize_export(cae_model_t *mm, const float *latents, int n, int hw, int32_t *symbols_host, int max_blocks,
                        void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !latents || !symbols_host) return fail(CAE_ERR_ARG, "NULL argument");
    if (m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if (n < 1 || hw < 1) return fail(CAE_ERR_ARG, "bad shape");
    {
        std::lock_guard<std::mutex> lk(m->mu);
        int rc = m->ensure_device();
        if (rc) return rc;
    }
    const size_t total = (size_t)n * m->c_bn * hw;
    // few, fat workgroups: a CU that hosts an export workgroup cannot host a workgroup of the register-file-filling
    // conv / deconv kernels, so the link is kept busy from as few CUs as possible
    const unsigned cap = (unsigned)std::max(max_blocks, 1);
    if (hw % 4 == 0 && (((uintptr_t)latents | (uintptr_t)symbols_host) & 15) == 0) {
        const size_t total4 = total / 4;
        const unsigned blocks = (unsigned)std::min<size_t>((total4 + 1023) / 1024, (size_t)cap);
        hipLaunchKernelGGL(quantize_export4_kernel, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, latents,
                           m->medians_dev.get<float>(), symbols_host, m->c_bn, hw / 4, total4);
    } else {
        const unsigned blocks = (unsigned)std::min<size_t>((total + 1023) / 1024, (size_t)cap);
        hipLaunchKernelGGL(quantize_kernel, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, latents, m->medians_dev.get<float>(),
                           symbols_host, m->c_bn, hw, total);
    }
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_dequantize(cae_model_t *mm, const int32_t *symbols, int n, int hw, float *latents, void *stream) {
    Model *m = reinterpret_cast<Model *>(mm);
    if (!m || !latents || !symbols) return fail(CAE_ERR_ARG, "NULL argument");
    if (m->ent.channels == 0) return fail(CAE_ERR_ARG, "entropy model not set");
    if (n < 1 || hw < 1) return fail(CAE_ERR_ARG, "bad shape");
    {
        std::lock_guard<std::mutex> lk(m->mu);
        int rc = m->ensure_device();
        if (rc) return rc;
    }
    const size_t total = (size_t)n * m->c_bn * hw;
    hipLaunchKernelGGL(dequantize_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, symbols,
                       m->medians_dev.get<float>(), latents, m->c_bn, hw, total);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // extern "C"
