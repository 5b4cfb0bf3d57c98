// What every entry point of the training C ABI (the product's cae_train.hip, included textually below) launches, on the
// CPU: the HIP host calls the file makes are replaced by recorders, the program links without the HIP runtime and never
// opens a GPU.  Per case it records one line per memset, launch, failure and return code -- the kernel by name, grid,
// block, dynamic LDS, every integer of the argument struct, every pointer by the role of the argument it equals -- and
// prints "case hash" (64-bit FNV-1a of the lines); with case names as arguments it prints those cases' lines in full.
// tests/test_train_launches.py compares the hashes with tests/golden/train_launches.json.  The program uses the C ABI
// and the kernel / struct names only, so the same file compiles against any revision of cae_train.hip.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

namespace th {

std::vector<std::string> g_events;
std::map<const void *, int> g_lds_limit;  // kernel -> largest hipFuncSetAttribute so far
int g_device = 0;                         // what hipGetDevice answers
bool g_malloc_fails = false;

void ev(const char *fmt, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_events.push_back(buf);
}

[[noreturn]] void die(const char *what) {
    fprintf(stderr, "train_launches: %s\n", what);
    for (size_t i = g_events.size() > 6 ? g_events.size() - 6 : 0; i < g_events.size(); ++i)
        fprintf(stderr, "  %s\n", g_events[i].c_str());
    exit(2);
}

// fake device pointers: one byte of an arena per role name, never dereferenced
char g_arena[64];
std::vector<std::string> g_roles;

void *ptr(const char *role) {
    for (size_t i = 0; i < g_roles.size(); ++i)
        if (g_roles[i] == role) return &g_arena[i];
    if (g_roles.size() == sizeof g_arena) die("too many pointer roles");
    g_roles.push_back(role);
    return &g_arena[g_roles.size() - 1];
}
template <class T>
T *P(const char *role) { return static_cast<T *>(ptr(role)); }

std::string role(const void *p) {
    if (!p) return "null";
    const char *c = static_cast<const char *>(p);
    if (c < g_arena || c >= g_arena + g_roles.size()) die("a pointer that is no argument reached a kernel");
    return g_roles[c - g_arena];
}

const char *kernel_name(const void *k);  // the table follows the product's code

// ---- the HIP host calls of cae_train.hip ----
hipError_t get_device(int *dev) {
    *dev = g_device;
    return hipSuccess;
}
hipError_t dev_malloc(void **p, size_t bytes) {
    if (g_malloc_fails) return hipErrorOutOfMemory;
    if (bytes < 1024) die("zero page smaller than 1 KiB");
    *p = ptr("zero");
    return hipSuccess;
}
hipError_t dev_memset(void *, int, size_t) { return hipSuccess; }
hipError_t dev_free(void *) { return hipSuccess; }
hipError_t last_error() { return hipSuccess; }
const char *error_string(hipError_t) { return "stubbed HIP error"; }
hipError_t func_set_attribute(const void *k, hipFuncAttribute attr, int bytes) {
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) die("unexpected function attribute");
    kernel_name(k);
    int &have = g_lds_limit[k];
    if (bytes > have) have = bytes;
    return hipSuccess;
}
hipError_t memset_async(void *p, int value, size_t bytes, hipStream_t) {
    ev("memset %s value=%d bytes=%zu", role(p).c_str(), value, bytes);
    return hipSuccess;
}

template <class K, class... A>
void launch(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args);

}  // namespace th

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) th::launch(__VA_ARGS__)
#define hipFuncSetAttribute th::func_set_attribute
#define hipMemsetAsync th::memset_async
#define hipGetDevice th::get_device
#define hipMalloc th::dev_malloc
#define hipMemset th::dev_memset
#define hipFree th::dev_free
#define hipGetLastError th::last_error
#define hipGetErrorString th::error_string

#include "cae_train.hip"

#undef hipMalloc
#undef hipFree

namespace cae {
int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    th::ev("fail %d %s", code, buf);
    return code;
}
}  // namespace cae

// the registration and launch calls the compiler emits for the kernels' host stubs: nothing to register, nothing runs
extern "C" {
void **__hipRegisterFatBinary(const void *) {
    static void *handle = nullptr;
    return &handle;
}
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
hipError_t __hipPopCallConfiguration(dim3 *, dim3 *, size_t *, hipStream_t *) { return hipSuccess; }
hipError_t hipLaunchKernel(const void *, dim3, dim3, void **, size_t, hipStream_t) { return hipSuccess; }
}

namespace th {

using namespace cae::tr;

#define TH_K(...) {(const void *)(__VA_ARGS__), #__VA_ARGS__}
const char *kernel_name(const void *k) {
    static const std::map<const void *, const char *> names = {
        TH_K(gather_gemm_kernel<1, false>), TH_K(gather_gemm_kernel<2, false>), TH_K(gather_gemm_kernel<3, false>),
        TH_K(gather_gemm_kernel<4, false>), TH_K(gather_gemm_kernel<5, false>), TH_K(gather_gemm_kernel<6, false>),
        TH_K(gather_gemm_kernel<1, true>), TH_K(gather_gemm_kernel<2, true>), TH_K(gather_gemm_kernel<3, true>),
        TH_K(gather_gemm_kernel<4, true>), TH_K(gather_gemm_kernel<5, true>), TH_K(gather_gemm_kernel<6, true>),
        TH_K(gg8_kernel<4, 2, 9>), TH_K(gg8_kernel<4, 4, 4>), TH_K(gg8_kernel<4, 4, 2>), TH_K(gg8_kernel<4, 4, 1>),
        TH_K(gg8_kernel<1, 4, 1>), TH_K(gg8_kernel<3, 2, 9>), TH_K(gg8_kernel<3, 4, 4>), TH_K(gg8_kernel<3, 4, 2>),
        TH_K(gg8_kernel<3, 4, 1>), TH_K(gg8t_kernel<false>), TH_K(gg8t_kernel<true>),
        TH_K(wgrad_kernel<1>), TH_K(wgrad_kernel<2>), TH_K(wgrad8_kernel),
        TH_K(gdn_gemm_a_kernel<1, 0>), TH_K(gdn_gemm_a_kernel<2, 0>), TH_K(gdn_gemm_a_kernel<3, 0>),
        TH_K(gdn_gemm_a_kernel<4, 0>), TH_K(gdn_gemm_a_kernel<5, 0>), TH_K(gdn_gemm_a_kernel<6, 0>),
        TH_K(gdn_gemm_a_kernel<1, 1>), TH_K(gdn_gemm_a_kernel<2, 1>), TH_K(gdn_gemm_a_kernel<3, 1>),
        TH_K(gdn_gemm_a_kernel<4, 1>), TH_K(gdn_gemm_a_kernel<5, 1>), TH_K(gdn_gemm_a_kernel<6, 1>),
        TH_K(gdn_gemm_a_kernel<1, 2>), TH_K(gdn_gemm_a_kernel<2, 2>), TH_K(gdn_gemm_a_kernel<3, 2>),
        TH_K(gdn_gemm_a_kernel<4, 2>), TH_K(gdn_gemm_a_kernel<5, 2>), TH_K(gdn_gemm_a_kernel<6, 2>),
        TH_K(gdn_gemm_b_kernel<1>), TH_K(gdn_gemm_b_kernel<2>), TH_K(gdn_gemm_b_kernel<3>),
        TH_K(gdn_gemm_b_kernel<4>), TH_K(gdn_gemm_b_kernel<5>), TH_K(gdn_gemm_b_kernel<6>),
        TH_K(gdn_fwd_fused_kernel<1>), TH_K(gdn_fwd_fused_kernel<2>), TH_K(gdn_fwd_fused_kernel<3>),
        TH_K(gdn_fwd_fused_kernel<4>), TH_K(gdn_bwd_fused_kernel<1>), TH_K(gdn_bwd_fused_kernel<2>),
        TH_K(gdn_bwd_fused_kernel<3>), TH_K(gdn_bwd_fused_kernel<4>),
        TH_K(pack_weights_kernel), TH_K(nchw_to_t_kernel), TH_K(t_to_nchw_kernel), TH_K(col2im_s1r_kernel),
        TH_K(im2col_s1r_kernel), TH_K(fold_acc_kernel), TH_K(pyramid_down_kernel), TH_K(im2col_s2_kernel),
        TH_K(col2im_s2_kernel), TH_K(fold_inplace_kernel), TH_K(act_bwd_kernel), TH_K(fold_to_bf16_kernel),
        TH_K(bn_moments_kernel), TH_K(bn_affine_kernel), TH_K(colsum_bf16_kernel),
    };
    auto it = names.find(k);
    if (it == names.end()) die("a launch or attribute call names a kernel the table does not know");
    return it->second;
}

// ---- one text per kernel argument ----
void add(std::string &s, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}
template <class T>
void add_list(std::string &s, const char *name, const T *v, int n) {
    add(s, " %s=", name);
    for (int i = 0; i < n; ++i) add(s, i ? ",%d" : "%d", (int)v[i]);
}
#define TH_I(f) add(s, " " #f "=%lld", (long long)a.f)
#define TH_P(f) add(s, " " #f "=%s", role(a.f).c_str())

void put(std::string &s, const FoldSrc &a) {
    add(s, " FoldSrc{");
    TH_P(g); TH_I(H); TH_I(W); TH_I(P);
    s += " }";
}
void put(std::string &s, const GGArgs &a) {
    s += " GGArgs{";
    TH_P(in); TH_P(out32); TH_P(out16); TH_P(wp); TH_P(bias); TH_P(zero);
    TH_I(N); TH_I(IH); TH_I(IW); TH_I(Ck); TH_I(Cn); TH_I(OH); TH_I(OW); TH_I(LH); TH_I(LW); TH_I(S); TH_I(SO); TH_I(oy0);
    TH_I(ox0); TH_I(reflect); TH_I(act); TH_I(ntaps); TH_I(ktaps); TH_I(dymin); TH_I(dxmin); TH_I(HR); TH_I(HC);
    TH_I(taps_per_stage); TH_I(m_plane); TH_I(m_hc); TH_I(nq); TH_I(npb); TH_I(nt0); TH_I(nt_all); TH_I(tiles_x);
    TH_I(tiles_y); TH_I(acc);
    add_list(s, "dy", a.dy, MAX_TAPS);
    add_list(s, "dx", a.dx, MAX_TAPS);
    add_list(s, "wt", a.wt, MAX_TAPS);
    s += " }";
}
void put(std::string &s, const WGArgs &a) {
    s += " WGArgs{";
    TH_P(x); TH_P(y); TH_P(gw); TH_P(zero);
    TH_I(N); TH_I(H); TH_I(W); TH_I(Ca); TH_I(OH); TH_I(OW); TH_I(Cb); TH_I(reflect); TH_I(m_hc); TH_I(m_ypp); TH_I(S);
    TH_I(kk); TH_I(dymin); TH_I(dxmin); TH_I(HR); TH_I(HC); TH_I(tiles_x); TH_I(tiles_y); TH_I(total_tiles); TH_I(cb0);
    TH_I(Cbs);
    add_list(s, "dy", a.dy, MAX_TAPS);
    add_list(s, "dx", a.dx, MAX_TAPS);
    s += " }";
}
void put(std::string &s, const GdnArgs &a) {
    s += " GdnArgs{";
    TH_P(a); TH_P(mat); TH_P(beta); TH_P(z);
    put(s, a.gy);
    TH_I(img_h); TH_I(img_w); TH_P(o32a); TH_P(o32b); TH_P(o16); TH_I(pixels); TH_I(C); TH_I(inverse);
    s += " }";
}
void put(std::string &s, const GdnFusedArgs &a) {
    s += " GdnFusedArgs{";
    TH_P(z); TH_P(gamma); TH_P(beta); TH_P(f); TH_P(y16);
    put(s, a.gy);
    TH_I(img_h); TH_I(img_w); TH_P(gz16); TH_P(ggamma); TH_P(gbeta); TH_I(pixels); TH_I(inverse);
    s += " }";
}
void put(std::string &s, int v) { add(s, " %d", v); }
void put(std::string &s, unsigned v) { add(s, " %u", v); }
void put(std::string &s, long v) { add(s, " %ld", v); }
void put(std::string &s, unsigned long v) { add(s, " %lu", v); }
void put(std::string &s, float v) { add(s, " %.9g", (double)v); }
template <class T>
void put(std::string &s, T *p) { add(s, " %s", role((const void *)p).c_str()); }

template <class K, class... A>
void launch(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t, A... args) {
    const void *k = (const void *)kern;
    std::string s;
    add(s, "launch %s grid=%u,%u,%u block=%u,%u,%u lds=%zu |", kernel_name(k), grid.x, grid.y, grid.z, block.x, block.y,
        block.z, lds);
    (put(s, args), ...);
    g_events.push_back(s);
    // the invariant outside the golden: dynamic LDS only after an attribute raise on this kernel to at least that size
    if (lds > 0 && (!g_lds_limit.count(k) || (size_t)g_lds_limit[k] < lds)) die("dynamic LDS above the kernel's raised limit");
    if ((size_t)grid.x * grid.y * grid.z == 0 || block.x * block.y * block.z == 0 || block.x * block.y * block.z > 1024)
        die("empty grid or bad block");
}

// ---- cases ----
struct Case {
    std::string name;
    std::function<void()> run;
};
std::vector<Case> g_cases;

std::string fmt(const char *f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
void add_case(const std::string &name, std::function<void()> run) { g_cases.push_back({name, std::move(run)}); }
// records an entry point's return value under a label that tells the calls of a case apart
void rc(const std::string &label, long long value) { ev("%s -> %lld", label.c_str(), value); }

const int C6[] = {32, 64, 96, 128, 160, 192};
struct Size { int h, w; };
const Size SIZES[] = {{2, 2}, {3, 4}, {37, 45}, {128, 128}, {256, 256}};
const int BATCHES[] = {1, 3, 16, 128};

#define IN P<void>("in")
#define PACKED P<void>("packed")
#define OUT32 P<float>("out32")
#define OUT16 P<void>("out16")
#define BIAS P<float>("bias")
#define STREAM P<void>("stream")

void conv_cases() {
    for (int ks : {3, 5})
        for (Size z : SIZES)
            for (int n : BATCHES) {
                const std::string tail = fmt("/k%d/%dx%d/n%d", ks, z.h, z.w, n);
                const int h = z.h, w = z.w, oh = (h + 1) / 2, ow = (w + 1) / 2;
                add_case("conv_forward_act" + tail, [=] {
                    for (int ck : C6)
                        for (int cn : C6)
                            rc(fmt("%d->%d", ck, cn), cae_t_conv_forward_act(IN, n, h, w, ck, PACKED, ks, OUT32, OUT16, cn, BIAS,
                                                                             (ck + cn) / 32 % 3, STREAM));
                });
                add_case("deconv_forward_act" + tail, [=] {
                    for (int ck : C6)
                        for (int cn : C6)
                            rc(fmt("%d->%d", ck, cn), cae_t_deconv_forward_act(IN, n, h, w, ck, PACKED, ks, OUT32, OUT16, cn,
                                                                               BIAS, (ck + cn) / 32 % 3, STREAM));
                });
                add_case("conv_dgrad_ext" + tail, [=] {  // (h, w): the layer's input; the gradient has (oh, ow)
                    for (int ck : C6)
                        for (int cn : C6)
                            rc(fmt("%d->%d", ck, cn),
                               cae_t_conv_dgrad_ext(IN, n, oh, ow, ck, PACKED, ks, h, w, OUT32, cn, STREAM));
                });
                add_case("deconv_dgrad" + tail, [=] {
                    for (int ck : C6)
                        for (int cn : C6)
                            rc(fmt("%d->%d", ck, cn),
                               cae_t_deconv_dgrad(IN, n, h, w, ck, PACKED, ks, OUT32, OUT16, cn, STREAM));
                });
            }
    // the forms without an activation argument, and one output only
    for (int ks : {3, 5})
        add_case(fmt("forward_plain/k%d", ks), [=] {
            for (int c : C6) {
                rc(fmt("conv %d", c), cae_t_conv_forward(IN, 3, 37, 45, c, PACKED, ks, OUT32, nullptr, c, nullptr, STREAM));
                rc(fmt("deconv %d", c), cae_t_deconv_forward(IN, 3, 37, 45, c, PACKED, ks, nullptr, OUT16, c, BIAS, STREAM));
                rc(fmt("conv 1x %d", c), cae_t_conv_forward(IN, 1, 2, 2, 192, PACKED, ks, nullptr, OUT16, c, BIAS, STREAM));
                rc(fmt("deconv 1x %d", c), cae_t_deconv_forward(IN, 1, 1, 1, c, PACKED, ks, OUT32, nullptr, 192, BIAS, STREAM));
            }
        });
    // a forced number of samples per block (gg8 only; gg8t keeps its own)
    add_case("samples_per_block", [] {
        rc("set -1", cae_t_set_samples_per_block(-1));
        rc("set 3", cae_t_set_samples_per_block(3));
        for (int n : BATCHES)
            for (int c : {32, 128, 192}) {
                rc(fmt("conv n%d %d", n, c), cae_t_conv_forward_act(IN, n, 64, 64, c, PACKED, 3, OUT32, OUT16, c, BIAS, 1, STREAM));
                rc(fmt("deconv n%d %d", n, c), cae_t_deconv_forward_act(IN, n, 32, 32, c, PACKED, 3, OUT32, OUT16, c, BIAS, 1, STREAM));
                rc(fmt("pointwise n%d %d", n, c), cae_t_pointwise(IN, n, 64, 64, c, PACKED, OUT32, OUT16, c, BIAS, 0, STREAM));
            }
        rc("set 0", cae_t_set_samples_per_block(0));
        rc("conv after", cae_t_conv_forward_act(IN, 16, 64, 64, 128, PACKED, 3, OUT32, OUT16, 128, BIAS, 1, STREAM));
    });
    for (int ks : {3, 5})
        for (int mode = 0; mode < 4; ++mode)
            for (Size z : {Size{1, 1}, Size{3, 4}, Size{37, 45}, Size{128, 128}, Size{256, 256}})
                add_case(fmt("corr_s1/k%d/mode%d/%dx%d", ks, mode, z.h, z.w), [=] {
                    for (int n : BATCHES)
                        for (int ck : C6)
                            for (int cn : {ck, 224 - ck})
                                for (int act = 0; act < 3; ++act)
                                    rc(fmt("n%d %d->%d act%d", n, ck, cn, act),
                                       cae_t_corr_s1(IN, n, z.h, z.w, ck, PACKED, ks, mode, OUT32, act ? OUT16 : nullptr, cn,
                                                     act == 2 ? nullptr : BIAS, act, STREAM));
                });
    for (Size z : {Size{1, 1}, Size{3, 4}, Size{37, 45}, Size{128, 128}, Size{256, 256}})
        add_case(fmt("pointwise/%dx%d", z.h, z.w), [=] {
            for (int n : BATCHES)
                for (int ck : C6)
                    for (int cn : C6) {
                        rc(fmt("n%d %d->%d", n, ck, cn), cae_t_pointwise(IN, n, z.h, z.w, ck, PACKED, OUT32, OUT16, cn, BIAS,
                                                                         (ck + cn) / 32 % 3, STREAM));
                        rc(fmt("acc n%d %d->%d", n, ck, cn), cae_t_pointwise_acc(IN, n, z.h, z.w, ck, PACKED, OUT32, cn, STREAM));
                        rc(fmt("wgrad n%d %dx%d", n, ck, cn),
                           cae_t_wgrad_pointwise(IN, P<void>("y16"), n, z.h, z.w, ck, cn, P<float>("gw32"), STREAM));
                    }
        });
}

void wgrad_cases() {
    for (int ks : {3, 5})
        for (int reflect : {0, 1})
            for (Size z : SIZES)
                add_case(fmt("wgrad/k%d/%s/%dx%d", ks, reflect ? "reflect" : "zero", z.h, z.w), [=] {
                    const int oh = (z.h + 1) / 2, ow = (z.w + 1) / 2;
                    for (int n : BATCHES)
                        for (int ca : C6)
                            for (int cb : C6) {
                                rc(fmt("s2 n%d %dx%d", n, ca, cb), cae_t_wgrad(IN, n, z.h, z.w, ca, P<void>("y16"), oh, ow, cb, ks,
                                                                               reflect, P<float>("gw32"), STREAM));
                                rc(fmt("s1 n%d %dx%d", n, ca, cb), cae_t_wgrad_s1(IN, n, z.h, z.w, ca, P<void>("y16"), cb, ks,
                                                                                  reflect, P<float>("gw32"), STREAM));
                            }
                    // the transposed layers' weight gradient: the large tensor is the gradient, twice the input
                    rc("deconv", cae_t_wgrad(IN, 16, 2 * z.h, 2 * z.w, 128, P<void>("y16"), z.h, z.w, 128, ks, 0,
                                             P<float>("gw32"), STREAM));
                });
}

void gdn_cases() {
    for (int pad : {0, 1, 2})
        for (Size z : {Size{1, 1}, Size{3, 4}, Size{37, 45}, Size{128, 128}})
            add_case(fmt("gdn/pad%d/%dx%d", pad, z.h, z.w), [=] {
                for (int n : BATCHES)
                    for (int c : C6)
                        for (int inverse : {0, 1}) {
                            const long pixels = (long)n * z.h * z.w;
                            const std::string tag = fmt("n%d c%d inv%d", n, c, inverse);
                            rc("forward " + tag, cae_t_gdn_forward(P<float>("z32"), pixels, c, P<float>("beta"), P<float>("gamma"),
                                                                  inverse, inverse ? nullptr : P<float>("y32"), P<void>("y16"),
                                                                  STREAM));
                            rc("backward " + tag,
                               cae_t_gdn_backward(P<float>("z32"), P<float>("gext32"), n, z.h, z.w, pad, c, P<float>("beta"),
                                                  P<float>("gamma"), P<float>("gamma_t"), inverse, P<float>("gn_ws32"),
                                                  P<float>("gzd_ws32"), inverse ? P<float>("gz32") : nullptr, P<void>("gz16"),
                                                  P<float>("ggamma"), P<float>("gbeta"), STREAM));
                            rc("saved_elems " + tag, (long long)cae_t_gdn_saved_elems(pixels, c));
                            rc("forward_save " + tag,
                               cae_t_gdn_forward_save(P<float>("z32"), pixels, c, P<float>("beta"), P<float>("gamma"), inverse,
                                                      P<void>("y16"), P<float>("f_saved"), STREAM));
                            rc("backward_fused " + tag,
                               cae_t_gdn_backward_fused(P<float>("z32"), P<float>("f_saved"), P<float>("gext32"), n, z.h, z.w, pad,
                                                        c, P<float>("gamma"), inverse, P<void>("gz16"), P<float>("ggamma"),
                                                        P<float>("gbeta"), STREAM));
                        }
            });
}

void elementwise_cases() {
    // ew_grid clamps at 8192 blocks of 256: (n, h, w) below and above it for every entry point
    for (Size z : {Size{3, 4}, Size{37, 45}, Size{256, 256}})
        for (int n : {1, 16, 128})
            add_case(fmt("elementwise/%dx%d/n%d", z.h, z.w, n), [=] {
                const int h = z.h, w = z.w;
                float *x = P<float>("x"), *out = P<float>("out");
                for (int ks : {1, 3, 5})
                    for (int contract : {0, 1}) {
                        rc(fmt("packed_bytes k%d", ks), (long long)cae_t_packed_bytes(3 + 61 * contract, 192 - 70 * contract, ks));
                        rc(fmt("pack k%d c%d", ks, contract),
                           cae_t_pack_weights(x, h * n, w + 29 * contract, ks, contract, PACKED, STREAM));
                    }
                rc("from_nchw", cae_t_from_nchw(x, n, 3, h, w, 32, OUT16, OUT32, STREAM));
                rc("from_nchw 16", cae_t_from_nchw(x, n, 40, h, w, 64, OUT16, nullptr, STREAM));
                rc("to_nchw", cae_t_to_nchw(OUT32, n, 3, h, w, 32, out, STREAM));
                for (int ks : {3, 5})
                    for (int c : {1, 3}) {
                        const int kp = (ks * ks * c + 31) / 32 * 32;
                        rc(fmt("col2im_s1r k%d c%d", ks, c), cae_t_col2im_s1r(OUT32, BIAS, n, c, h, w, ks, kp, out, STREAM));
                        rc(fmt("im2col_s1r k%d c%d", ks, c), cae_t_im2col_s1r(x, n, c, h, w, ks, kp, OUT16, STREAM));
                        const int c2 = ks == 3 ? c : 1;
                        rc(fmt("im2col_s2 k%d c%d", ks, c2),
                           cae_t_im2col_s2(x, n, c2, h, w, (h + 1) / 2, (w + 1) / 2, ks, c & 1, OUT16, STREAM));
                        rc(fmt("col2im_s2 k%d c%d", ks, c2), cae_t_col2im_s2(OUT32, c == 1 ? nullptr : BIAS, n, c2, h, w, ks, out, STREAM));
                    }
                for (int pad : {0, 1, 2})
                    for (int cp : {32, 192}) {
                        const std::string tag = fmt("pad%d c%d", pad, cp);
                        rc("fold_acc " + tag, cae_t_fold_acc(P<float>("gext32"), n, h, w, pad, cp, OUT32, STREAM));
                        rc("fold_to_bf16 " + tag, cae_t_fold_to_bf16(P<float>("gext32"), n, h, w, pad, cp, OUT16, STREAM));
                        for (int act : {1, 2}) {
                            rc(fmt("act_backward ext act%d ", act) + tag,
                               cae_t_act_backward(nullptr, P<float>("gext32"), pad, P<void>("y16"), n, h, w, cp, act, OUT16, STREAM));
                            rc(fmt("act_backward g16 act%d ", act) + tag,
                               cae_t_act_backward(P<void>("g16"), P<float>("gext32"), pad, P<void>("y16"), n, h, w, cp, act, OUT16,
                                                  STREAM));
                        }
                    }
                rc("pyramid_down", cae_t_pyramid_down(x, n, 3, h, w, out, STREAM));
                for (int c : {1, 3, 192, 2048}) {
                    rc(fmt("bn_moments c%d", c), cae_t_bn_moments(P<float>("a"), P<float>("b"), n, c, (long)h * w, P<double>("s1"),
                                                                  P<double>("s2"), STREAM));
                    rc(fmt("bn_affine c%d", c), cae_t_bn_affine(P<float>("a"), c == 3 ? nullptr : P<float>("b"), n, c, (long)h * w,
                                                                P<float>("A"), c == 3 ? nullptr : P<float>("B"), P<float>("C"), out,
                                                                STREAM));
                }
                for (int cp : {32, 96, 256}) rc(fmt("colsum c%d", cp), cae_t_colsum(P<void>("g16"), (long)n * h * w, cp, out, STREAM));
            });
}

void rejection_cases() {
    add_case("reject/null", [] {
        void *in = IN, *pk = PACKED, *o16 = OUT16, *y16 = P<void>("y16");
        float *o32 = OUT32, *f = P<float>("x");
        double *d = P<double>("s1");
        rc("pack w", cae_t_pack_weights(nullptr, 4, 4, 3, 0, pk, STREAM));
        rc("pack packed", cae_t_pack_weights(f, 4, 4, 3, 0, nullptr, STREAM));
        rc("from_nchw x", cae_t_from_nchw(nullptr, 1, 3, 4, 4, 32, o16, o32, STREAM));
        rc("from_nchw out", cae_t_from_nchw(f, 1, 3, 4, 4, 32, nullptr, nullptr, STREAM));
        rc("to_nchw t", cae_t_to_nchw(nullptr, 1, 3, 4, 4, 32, f, STREAM));
        rc("to_nchw out", cae_t_to_nchw(o32, 1, 3, 4, 4, 32, nullptr, STREAM));
        rc("conv x", cae_t_conv_forward(nullptr, 1, 4, 4, 32, pk, 3, o32, o16, 32, nullptr, STREAM));
        rc("conv packed", cae_t_conv_forward(in, 1, 4, 4, 32, nullptr, 3, o32, o16, 32, nullptr, STREAM));
        rc("conv out", cae_t_conv_forward(in, 1, 4, 4, 32, pk, 3, nullptr, nullptr, 32, nullptr, STREAM));
        rc("conv_act x", cae_t_conv_forward_act(nullptr, 1, 4, 4, 32, pk, 3, o32, o16, 32, nullptr, 1, STREAM));
        rc("conv_act out", cae_t_conv_forward_act(in, 1, 4, 4, 32, pk, 3, nullptr, nullptr, 32, nullptr, 1, STREAM));
        rc("deconv x", cae_t_deconv_forward(nullptr, 1, 4, 4, 32, pk, 3, o32, o16, 32, nullptr, STREAM));
        rc("deconv out", cae_t_deconv_forward(in, 1, 4, 4, 32, pk, 3, nullptr, nullptr, 32, nullptr, STREAM));
        rc("deconv_act packed", cae_t_deconv_forward_act(in, 1, 4, 4, 32, nullptr, 3, o32, o16, 32, nullptr, 1, STREAM));
        rc("deconv_act out", cae_t_deconv_forward_act(in, 1, 4, 4, 32, pk, 3, nullptr, nullptr, 32, nullptr, 1, STREAM));
        rc("corr_s1 x", cae_t_corr_s1(nullptr, 1, 4, 4, 32, pk, 3, 0, o32, o16, 32, nullptr, 0, STREAM));
        rc("corr_s1 out", cae_t_corr_s1(in, 1, 4, 4, 32, pk, 3, 0, nullptr, nullptr, 32, nullptr, 0, STREAM));
        rc("pointwise packed", cae_t_pointwise(in, 1, 4, 4, 32, nullptr, o32, o16, 32, nullptr, 0, STREAM));
        rc("pointwise out", cae_t_pointwise(in, 1, 4, 4, 32, pk, nullptr, nullptr, 32, nullptr, 0, STREAM));
        rc("pointwise_acc out", cae_t_pointwise_acc(in, 1, 4, 4, 32, pk, nullptr, 32, STREAM));
        rc("col2im_s1r u", cae_t_col2im_s1r(nullptr, nullptr, 1, 3, 4, 4, 3, 32, f, STREAM));
        rc("col2im_s1r out", cae_t_col2im_s1r(o32, nullptr, 1, 3, 4, 4, 3, 32, nullptr, STREAM));
        rc("im2col_s1r g", cae_t_im2col_s1r(nullptr, 1, 3, 4, 4, 3, 32, o16, STREAM));
        rc("im2col_s1r out", cae_t_im2col_s1r(f, 1, 3, 4, 4, 3, 32, nullptr, STREAM));
        rc("fold_acc g", cae_t_fold_acc(nullptr, 1, 4, 4, 1, 32, o32, STREAM));
        rc("fold_acc out", cae_t_fold_acc(o32, 1, 4, 4, 1, 32, nullptr, STREAM));
        rc("pyramid x", cae_t_pyramid_down(nullptr, 1, 3, 4, 4, f, STREAM));
        rc("pyramid out", cae_t_pyramid_down(f, 1, 3, 4, 4, nullptr, STREAM));
        rc("wgrad_pointwise x", cae_t_wgrad_pointwise(nullptr, y16, 1, 4, 4, 32, 32, f, STREAM));
        rc("wgrad y", cae_t_wgrad(in, 1, 4, 4, 32, nullptr, 2, 2, 32, 3, 1, f, STREAM));
        rc("wgrad_s1 gw", cae_t_wgrad_s1(in, 1, 4, 4, 32, y16, 32, 3, 1, nullptr, STREAM));
        rc("im2col_s2 x", cae_t_im2col_s2(nullptr, 1, 3, 4, 4, 2, 2, 3, 1, o16, STREAM));
        rc("im2col_s2 out", cae_t_im2col_s2(f, 1, 3, 4, 4, 2, 2, 3, 1, nullptr, STREAM));
        rc("col2im_s2 u", cae_t_col2im_s2(nullptr, nullptr, 1, 3, 4, 4, 3, f, STREAM));
        rc("col2im_s2 out", cae_t_col2im_s2(o32, nullptr, 1, 3, 4, 4, 3, nullptr, STREAM));
        rc("act_backward g", cae_t_act_backward(nullptr, nullptr, 1, y16, 1, 4, 4, 32, 1, o16, STREAM));
        rc("act_backward y", cae_t_act_backward(in, nullptr, 1, nullptr, 1, 4, 4, 32, 1, o16, STREAM));
        rc("act_backward out", cae_t_act_backward(in, nullptr, 1, y16, 1, 4, 4, 32, 1, nullptr, STREAM));
        rc("dgrad_ext g", cae_t_conv_dgrad_ext(nullptr, 1, 2, 2, 32, pk, 3, 4, 4, o32, 32, STREAM));
        rc("dgrad_ext out", cae_t_conv_dgrad_ext(in, 1, 2, 2, 32, pk, 3, 4, 4, nullptr, 32, STREAM));
        rc("deconv_dgrad packed", cae_t_deconv_dgrad(in, 1, 2, 2, 32, nullptr, 3, o32, o16, 32, STREAM));
        rc("deconv_dgrad out", cae_t_deconv_dgrad(in, 1, 2, 2, 32, pk, 3, nullptr, nullptr, 32, STREAM));
        rc("gdn_forward z", cae_t_gdn_forward(nullptr, 16, 32, f, f, 0, o32, o16, STREAM));
        rc("gdn_forward beta", cae_t_gdn_forward(o32, 16, 32, nullptr, f, 0, o32, o16, STREAM));
        rc("gdn_forward out", cae_t_gdn_forward(o32, 16, 32, f, f, 0, nullptr, nullptr, STREAM));
        rc("gdn_backward gamma_t", cae_t_gdn_backward(f, f, 1, 4, 4, 1, 32, f, f, nullptr, 0, f, f, o32, o16, f, f, STREAM));
        rc("gdn_backward gz", cae_t_gdn_backward(f, f, 1, 4, 4, 1, 32, f, f, f, 0, f, f, nullptr, nullptr, f, f, STREAM));
        rc("gdn_backward gbeta", cae_t_gdn_backward(f, f, 1, 4, 4, 1, 32, f, f, f, 0, f, f, o32, o16, f, nullptr, STREAM));
        rc("gdn_forward_save y16", cae_t_gdn_forward_save(f, 16, 32, f, f, 0, nullptr, f, STREAM));
        rc("gdn_forward_save f", cae_t_gdn_forward_save(f, 16, 32, f, f, 0, o16, nullptr, STREAM));
        rc("gdn_backward_fused gext", cae_t_gdn_backward_fused(f, f, nullptr, 1, 4, 4, 1, 32, f, 0, o16, f, f, STREAM));
        rc("gdn_backward_fused ggamma", cae_t_gdn_backward_fused(f, f, f, 1, 4, 4, 1, 32, f, 0, o16, nullptr, f, STREAM));
        rc("fold_to_bf16 g", cae_t_fold_to_bf16(nullptr, 1, 4, 4, 1, 32, o16, STREAM));
        rc("fold_to_bf16 out", cae_t_fold_to_bf16(f, 1, 4, 4, 1, 32, nullptr, STREAM));
        rc("bn_moments s2", cae_t_bn_moments(f, f, 1, 3, 16, d, nullptr, STREAM));
        rc("bn_moments b", cae_t_bn_moments(f, nullptr, 1, 3, 16, d, d, STREAM));
        rc("bn_affine b without B", cae_t_bn_affine(f, f, 1, 3, 16, f, nullptr, f, f, STREAM));
        rc("bn_affine out", cae_t_bn_affine(f, nullptr, 1, 3, 16, f, nullptr, f, nullptr, STREAM));
        rc("colsum g", cae_t_colsum(nullptr, 16, 32, f, STREAM));
        rc("colsum out", cae_t_colsum(in, 16, 32, nullptr, STREAM));
    });
    add_case("reject/channels", [] {
        float *f = P<float>("x");
        for (int c : {0, 16, 33, 224, 256}) {
            rc(fmt("conv ck %d", c), cae_t_conv_forward_act(IN, 1, 8, 8, c, PACKED, 3, OUT32, OUT16, 32, BIAS, 0, STREAM));
            rc(fmt("conv cn %d", c), cae_t_conv_forward_act(IN, 1, 8, 8, 32, PACKED, 5, OUT32, OUT16, c, BIAS, 0, STREAM));
            rc(fmt("deconv ck %d", c), cae_t_deconv_forward_act(IN, 1, 8, 8, c, PACKED, 3, OUT32, OUT16, 64, BIAS, 0, STREAM));
            rc(fmt("deconv cn %d", c), cae_t_deconv_forward_act(IN, 1, 8, 8, 64, PACKED, 3, OUT32, OUT16, c, BIAS, 0, STREAM));
            rc(fmt("deconv k5 cn %d", c), cae_t_deconv_forward(IN, 1, 8, 8, 64, PACKED, 5, OUT32, OUT16, c, BIAS, STREAM));
            rc(fmt("dgrad_ext ck %d", c), cae_t_conv_dgrad_ext(IN, 1, 4, 4, c, PACKED, 3, 8, 8, OUT32, 64, STREAM));
            rc(fmt("dgrad_ext cn %d", c), cae_t_conv_dgrad_ext(IN, 1, 4, 4, 64, PACKED, 3, 8, 8, OUT32, c, STREAM));
            rc(fmt("deconv_dgrad cn %d", c), cae_t_deconv_dgrad(IN, 1, 4, 4, 64, PACKED, 3, OUT32, OUT16, c, STREAM));
            rc(fmt("corr_s1 ck %d", c), cae_t_corr_s1(IN, 1, 8, 8, c, PACKED, 3, 0, OUT32, OUT16, 32, BIAS, 0, STREAM));
            rc(fmt("pointwise cn %d", c), cae_t_pointwise(IN, 1, 8, 8, 32, PACKED, OUT32, OUT16, c, BIAS, 0, STREAM));
            rc(fmt("pointwise_acc ck %d", c), cae_t_pointwise_acc(IN, 1, 8, 8, c, PACKED, OUT32, 32, STREAM));
            rc(fmt("wgrad ca %d", c), cae_t_wgrad(IN, 1, 8, 8, c, P<void>("y16"), 4, 4, 32, 3, 1, P<float>("gw32"), STREAM));
            rc(fmt("wgrad cb %d", c), cae_t_wgrad(IN, 1, 8, 8, 32, P<void>("y16"), 4, 4, c, 3, 1, P<float>("gw32"), STREAM));
            rc(fmt("wgrad_s1 cb %d", c), cae_t_wgrad_s1(IN, 1, 8, 8, 32, P<void>("y16"), c, 3, 1, P<float>("gw32"), STREAM));
            rc(fmt("wgrad_pointwise ca %d", c), cae_t_wgrad_pointwise(IN, P<void>("y16"), 1, 8, 8, c, 32, P<float>("gw32"), STREAM));
            rc(fmt("gdn_forward %d", c), cae_t_gdn_forward(f, 64, c, f, f, 0, OUT32, OUT16, STREAM));
            rc(fmt("gdn_backward %d", c), cae_t_gdn_backward(f, f, 1, 8, 8, 1, c, f, f, f, 0, f, f, OUT32, OUT16, f, f, STREAM));
            rc(fmt("gdn_forward_save %d", c), cae_t_gdn_forward_save(f, 64, c, f, f, 0, OUT16, f, STREAM));
            rc(fmt("gdn_backward_fused %d", c), cae_t_gdn_backward_fused(f, f, f, 1, 8, 8, 1, c, f, 0, OUT16, f, f, STREAM));
            rc(fmt("saved_elems %d", c), (long long)cae_t_gdn_saved_elems(64, c));
            rc(fmt("from_nchw %d", c), cae_t_from_nchw(f, 1, 3, 8, 8, c, OUT16, OUT32, STREAM));
            rc(fmt("to_nchw %d", c), cae_t_to_nchw(OUT32, 1, 3, 8, 8, c, f, STREAM));
            rc(fmt("fold_acc %d", c), cae_t_fold_acc(f, 1, 8, 8, 1, c, OUT32, STREAM));
            rc(fmt("fold_to_bf16 %d", c), cae_t_fold_to_bf16(f, 1, 8, 8, 1, c, OUT16, STREAM));
            rc(fmt("act_backward %d", c), cae_t_act_backward(IN, nullptr, 0, P<void>("y16"), 1, 8, 8, c, 1, OUT16, STREAM));
            rc(fmt("colsum %d", c), cae_t_colsum(IN, 64, c + 64, f, STREAM));
        }
        for (int c : {160, 192}) {  // the fused GDN kernels stop at 128 channels
            rc(fmt("gdn_forward_save %d", c), cae_t_gdn_forward_save(f, 64, c, f, f, 0, OUT16, f, STREAM));
            rc(fmt("gdn_backward_fused %d", c), cae_t_gdn_backward_fused(f, f, f, 1, 8, 8, 1, c, f, 0, OUT16, f, f, STREAM));
            rc(fmt("saved_elems %d", c), (long long)cae_t_gdn_saved_elems(64, c));
        }
    });
    add_case("reject/kernel_size_mode_act", [] {
        for (int ks : {0, 1, 2, 4, 7}) {
            rc(fmt("conv k%d", ks), cae_t_conv_forward_act(IN, 1, 8, 8, 32, PACKED, ks, OUT32, OUT16, 32, BIAS, 0, STREAM));
            rc(fmt("deconv k%d", ks), cae_t_deconv_forward_act(IN, 1, 8, 8, 64, PACKED, ks, OUT32, OUT16, 64, BIAS, 0, STREAM));
            rc(fmt("dgrad_ext k%d", ks), cae_t_conv_dgrad_ext(IN, 1, 4, 4, 64, PACKED, ks, 8, 8, OUT32, 64, STREAM));
            rc(fmt("deconv_dgrad k%d", ks), cae_t_deconv_dgrad(IN, 1, 4, 4, 64, PACKED, ks, OUT32, OUT16, 64, STREAM));
            rc(fmt("corr_s1 k%d", ks), cae_t_corr_s1(IN, 1, 8, 8, 32, PACKED, ks, 1, OUT32, OUT16, 32, BIAS, 0, STREAM));
            rc(fmt("wgrad k%d", ks), cae_t_wgrad(IN, 1, 8, 8, 32, P<void>("y16"), 4, 4, 32, ks, 1, P<float>("gw32"), STREAM));
            rc(fmt("wgrad_s1 k%d", ks), cae_t_wgrad_s1(IN, 1, 8, 8, 32, P<void>("y16"), 32, ks, 0, P<float>("gw32"), STREAM));
            rc(fmt("col2im_s1r k%d", ks), cae_t_col2im_s1r(OUT32, BIAS, 1, 3, 8, 8, ks, 96, P<float>("out"), STREAM));
            rc(fmt("im2col_s1r k%d", ks), cae_t_im2col_s1r(P<float>("x"), 1, 3, 8, 8, ks, 96, OUT16, STREAM));
            rc(fmt("im2col_s2 k%d", ks), cae_t_im2col_s2(P<float>("x"), 1, 1, 8, 8, 4, 4, ks, 1, OUT16, STREAM));
            rc(fmt("col2im_s2 k%d", ks), cae_t_col2im_s2(OUT32, BIAS, 1, 1, 8, 8, ks, P<float>("out"), STREAM));
        }
        for (int mode : {-1, 4}) rc(fmt("corr_s1 mode %d", mode), cae_t_corr_s1(IN, 1, 8, 8, 32, PACKED, 3, mode, OUT32, OUT16, 32, BIAS, 0, STREAM));
        for (int act : {-1, 3}) {
            rc(fmt("conv act %d", act), cae_t_conv_forward_act(IN, 1, 8, 8, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, act, STREAM));
            rc(fmt("deconv act %d", act), cae_t_deconv_forward_act(IN, 1, 8, 8, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, act, STREAM));
            rc(fmt("corr_s1 act %d", act), cae_t_corr_s1(IN, 1, 8, 8, 32, PACKED, 3, 0, OUT32, OUT16, 32, BIAS, act, STREAM));
            rc(fmt("pointwise act %d", act), cae_t_pointwise(IN, 1, 8, 8, 32, PACKED, OUT32, OUT16, 32, BIAS, act, STREAM));
        }
        for (int act : {0, 3}) rc(fmt("act_backward act %d", act), cae_t_act_backward(IN, nullptr, 0, P<void>("y16"), 1, 8, 8, 32, act, OUT16, STREAM));
    });
    add_case("reject/shapes", [] {
        float *f = P<float>("x");
        rc("conv n0", cae_t_conv_forward(IN, 0, 8, 8, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, STREAM));
        rc("conv h1", cae_t_conv_forward(IN, 1, 1, 8, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, STREAM));
        rc("conv_act w1", cae_t_conv_forward_act(IN, 1, 8, 1, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, 0, STREAM));
        rc("deconv h0", cae_t_deconv_forward(IN, 1, 0, 8, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, STREAM));
        rc("deconv_act n0", cae_t_deconv_forward_act(IN, 0, 8, 8, 32, PACKED, 3, OUT32, OUT16, 32, BIAS, 0, STREAM));
        rc("corr_s1 w0", cae_t_corr_s1(IN, 1, 8, 0, 32, PACKED, 3, 0, OUT32, OUT16, 32, BIAS, 0, STREAM));
        rc("pointwise n0", cae_t_pointwise(IN, 0, 8, 8, 32, PACKED, OUT32, OUT16, 32, BIAS, 0, STREAM));
        rc("pointwise_acc h0", cae_t_pointwise_acc(IN, 1, 0, 8, 32, PACKED, OUT32, 32, STREAM));
        rc("wgrad_pointwise n0", cae_t_wgrad_pointwise(IN, P<void>("y16"), 0, 8, 8, 32, 32, P<float>("gw32"), STREAM));
        // the gradient of a strided layer has ceil(h / 2) x ceil(w / 2) positions
        rc("dgrad_ext oh", cae_t_conv_dgrad_ext(IN, 1, 5, 4, 32, PACKED, 3, 8, 8, OUT32, 32, STREAM));
        rc("dgrad_ext ow", cae_t_conv_dgrad_ext(IN, 1, 4, 3, 32, PACKED, 3, 8, 8, OUT32, 32, STREAM));
        rc("dgrad_ext odd ok", cae_t_conv_dgrad_ext(IN, 1, 4, 5, 32, PACKED, 3, 7, 9, OUT32, 32, STREAM));
        rc("deconv_dgrad h0", cae_t_deconv_dgrad(IN, 1, 0, 4, 32, PACKED, 3, OUT32, OUT16, 32, STREAM));
        rc("wgrad 2oh<h", cae_t_wgrad(IN, 1, 9, 8, 32, P<void>("y16"), 4, 4, 32, 3, 1, P<float>("gw32"), STREAM));
        rc("wgrad 2ow<w", cae_t_wgrad(IN, 1, 8, 9, 32, P<void>("y16"), 4, 4, 32, 3, 1, P<float>("gw32"), STREAM));
        rc("wgrad oh0", cae_t_wgrad(IN, 1, 0, 8, 32, P<void>("y16"), 0, 4, 32, 3, 1, P<float>("gw32"), STREAM));
        rc("wgrad_s1 n0", cae_t_wgrad_s1(IN, 0, 8, 8, 32, P<void>("y16"), 32, 3, 1, P<float>("gw32"), STREAM));
        rc("pack dims", cae_t_pack_weights(f, 0, 4, 3, 0, PACKED, STREAM));
        rc("pack contract", cae_t_pack_weights(f, 4, 4, 3, 2, PACKED, STREAM));
        rc("from_nchw cp<c", cae_t_from_nchw(f, 1, 40, 8, 8, 32, OUT16, OUT32, STREAM));
        rc("to_nchw n0", cae_t_to_nchw(OUT32, 0, 3, 8, 8, 32, f, STREAM));
        rc("col2im_s1r c4", cae_t_col2im_s1r(OUT32, BIAS, 1, 4, 8, 8, 3, 64, f, STREAM));
        rc("col2im_s1r kp small", cae_t_col2im_s1r(OUT32, BIAS, 1, 3, 8, 8, 5, 64, f, STREAM));
        rc("col2im_s1r kp 128", cae_t_col2im_s1r(OUT32, BIAS, 1, 3, 8, 8, 5, 128, f, STREAM));
        rc("col2im_s1r image", cae_t_col2im_s1r(OUT32, BIAS, 1, 3, 2, 8, 5, 96, f, STREAM));
        rc("im2col_s1r kp", cae_t_im2col_s1r(f, 1, 3, 8, 8, 3, 40, OUT16, STREAM));
        rc("im2col_s1r image", cae_t_im2col_s1r(f, 1, 3, 8, 1, 3, 32, OUT16, STREAM));
        rc("fold_acc h<=pad", cae_t_fold_acc(f, 1, 2, 8, 2, 32, OUT32, STREAM));
        rc("fold_acc pad<0", cae_t_fold_acc(f, 1, 8, 8, -1, 32, OUT32, STREAM));
        rc("pyramid h1", cae_t_pyramid_down(f, 1, 3, 1, 8, f, STREAM));
        rc("im2col_s2 k5 c2", cae_t_im2col_s2(f, 1, 2, 8, 8, 4, 4, 5, 1, OUT16, STREAM));
        rc("im2col_s2 oh0", cae_t_im2col_s2(f, 1, 1, 8, 8, 0, 4, 3, 1, OUT16, STREAM));
        rc("col2im_s2 k3 c4", cae_t_col2im_s2(OUT32, BIAS, 1, 4, 8, 8, 3, f, STREAM));
        rc("act_backward pad<0", cae_t_act_backward(nullptr, f, -1, P<void>("y16"), 1, 8, 8, 32, 1, OUT16, STREAM));
        rc("gdn_forward pixels0", cae_t_gdn_forward(f, 0, 32, f, f, 0, OUT32, OUT16, STREAM));
        rc("gdn_backward pad<0", cae_t_gdn_backward(f, f, 1, 8, 8, -1, 32, f, f, f, 0, f, f, OUT32, OUT16, f, f, STREAM));
        rc("gdn_backward_fused n0", cae_t_gdn_backward_fused(f, f, f, 0, 8, 8, 1, 32, f, 0, OUT16, f, f, STREAM));
        rc("gdn_forward_save pixels0", cae_t_gdn_forward_save(f, 0, 32, f, f, 0, OUT16, f, STREAM));
        rc("saved_elems pixels0", (long long)cae_t_gdn_saved_elems(0, 32));
        rc("fold_to_bf16 w0", cae_t_fold_to_bf16(f, 1, 8, 0, 1, 32, OUT16, STREAM));
        rc("bn_moments c65536", cae_t_bn_moments(f, f, 1, 65536, 16, P<double>("s1"), P<double>("s2"), STREAM));
        rc("bn_moments hw0", cae_t_bn_moments(f, f, 1, 3, 0, P<double>("s1"), P<double>("s2"), STREAM));
        rc("bn_affine n0", cae_t_bn_affine(f, nullptr, 0, 3, 16, f, nullptr, f, f, STREAM));
        rc("colsum pixels0", cae_t_colsum(IN, 0, 32, f, STREAM));
        // 2^31 pixels and one below
        rc("gdn_backward 2^31", cae_t_gdn_backward(f, f, 128, 4096, 4096, 1, 32, f, f, f, 0, f, f, OUT32, OUT16, f, f, STREAM));
        rc("gdn_backward 2^31-4096", cae_t_gdn_backward(f, f, 1, 4096, 524287, 1, 32, f, f, f, 0, f, f, OUT32, OUT16, f, f, STREAM));
        rc("gdn_backward_fused 2^31", cae_t_gdn_backward_fused(f, f, f, 128, 4096, 4096, 1, 32, f, 0, OUT16, f, f, STREAM));
        rc("gdn_backward_fused 2^31-4096", cae_t_gdn_backward_fused(f, f, f, 1, 4096, 524287, 1, 32, f, 0, OUT16, f, f, STREAM));
        rc("gdn_forward_save 2^31", cae_t_gdn_forward_save(f, 1l << 31, 32, f, f, 0, OUT16, f, STREAM));
        rc("gdn_forward_save 2^31-1", cae_t_gdn_forward_save(f, (1l << 31) - 1, 32, f, f, 0, OUT16, f, STREAM));
        rc("gdn_forward 2^31", cae_t_gdn_forward(f, 1l << 31, 32, f, f, 0, OUT32, OUT16, STREAM));
    });
    // a device whose zero page cannot be allocated: every convolution product answers CAE_ERR_NOMEM and launches nothing
    add_case("reject/no_zero_page", [] {
        g_device = 1;
        g_malloc_fails = true;
        for (int ks : {3, 5})
            for (int c : {64, 96}) {
                const std::string tag = fmt("k%d c%d", ks, c);
                rc("conv " + tag, cae_t_conv_forward_act(IN, 1, 8, 8, c, PACKED, ks, OUT32, OUT16, c, BIAS, 0, STREAM));
                rc("deconv " + tag, cae_t_deconv_forward_act(IN, 1, 8, 8, c, PACKED, ks, OUT32, OUT16, c, BIAS, 0, STREAM));
                rc("dgrad_ext " + tag, cae_t_conv_dgrad_ext(IN, 1, 4, 4, c, PACKED, ks, 8, 8, OUT32, c, STREAM));
                rc("deconv_dgrad " + tag, cae_t_deconv_dgrad(IN, 1, 4, 4, c, PACKED, ks, OUT32, OUT16, c, STREAM));
                rc("corr_s1 " + tag, cae_t_corr_s1(IN, 1, 8, 8, c, PACKED, ks, 2, OUT32, OUT16, c, BIAS, 0, STREAM));
                rc("wgrad " + tag, cae_t_wgrad(IN, 1, 8, 8, c, P<void>("y16"), 4, 4, c, ks, 1, P<float>("gw32"), STREAM));
            }
        rc("pointwise", cae_t_pointwise(IN, 1, 8, 8, 64, PACKED, OUT32, OUT16, 64, BIAS, 0, STREAM));
        rc("wgrad_pointwise", cae_t_wgrad_pointwise(IN, P<void>("y16"), 1, 8, 8, 64, 64, P<float>("gw32"), STREAM));
        g_device = 0;
        g_malloc_fails = false;
    });
}

}  // namespace th

int main(int argc, char **argv) {
    using namespace th;
    ptr("zero");  // (role 0, whichever case allocates the page first)
    conv_cases();
    wgrad_cases();
    gdn_cases();
    elementwise_cases();
    rejection_cases();
    int printed = 0;
    for (const Case &c : g_cases) {
        g_events.clear();
        c.run();
        bool full = false;
        for (int i = 1; i < argc; ++i) full = full || c.name == argv[i];
        if (argc > 1 && !full) continue;
        ++printed;
        if (full) {
            printf("== %s\n", c.name.c_str());
            for (const std::string &e : g_events) printf("%s\n", e.c_str());
            continue;
        }
        uint64_t h = 0xcbf29ce484222325ull;
        for (const std::string &e : g_events) {
            for (unsigned char ch : e) h = (h ^ ch) * 0x100000001b3ull;
            h = (h ^ '\n') * 0x100000001b3ull;
        }
        printf("%s %016llx\n", c.name.c_str(), (unsigned long long)h);
    }
    if (argc > 1 && printed != argc - 1) die("unknown case name");
    return 0;
}
