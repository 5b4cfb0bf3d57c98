// Internal types of libcae_hip.so (not part of the ABI).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <utility>
#include <vector>

namespace cae {

int fail(int code, const char *fmt, ...);

// hipFree; defined with the HIP half of the library (cae_api.hip) so that this header needs no HIP include
void dev_free(void *p);

// Owner of one device allocation: move-only, frees in its destructor.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p, o.p);
            std::swap(bytes, o.bytes);
        }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) dev_free(p);
        p = nullptr;
        bytes = 0;
    }
    explicit operator bool() const { return p != nullptr; }
    template <class T>
    T *get() const { return static_cast<T *>(p); }
    int alloc(size_t n);                    // a fresh, uninitialised allocation of n bytes (frees the previous one first)
    int upload(const void *src, size_t n);  // a fresh allocation holding a copy of src[0..n) (blocking)
    template <class T>
    int upload(const std::vector<T> &v) { return upload(v.data(), v.size() * sizeof(T)); }
};

struct Layer {
    bool set = false;
    int cin = 0, cout = 0, ct = 0, chunks = 0;
    bool gdn = false;
    DevBuf wp;       // packed weights
    DevBuf bias;     // [ct*32] or null
    DevBuf gp;       // packed gamma
    DevBuf beta;     // [ct*32]
    DevBuf wp_edge;  // packed weights of the specialised first-conv / last-deconv kernel, or null
    // LeakyReLU / ReLU units: stride-1 convolution (cin -> cin) + activation in front of the strided one
    // stride-1 (transposed) convolutions cin -> cin in front of the strided layer: the pre-convolution of the
    // LeakyReLU / ReLU units and the res_model of the residual units (_autoencoders.py:62-76, :104-174, :230-304)
    struct Stage {
        DevBuf wp, bias, gp, beta;
        DevBuf wp16;           // f16x3 path: packed hi/lo weights
        DevBuf gp16;           // f16x3 path: packed hi/lo gamma (GDN / IGDN stages of residual units)
        bool gdn = false;      // GDN (analysis) / IGDN (synthesis) after the convolution, else `act`
        int act = 0;
        bool add_res = false;  // + the unit's input after the activation (residual units)
        int post_act = 0;      // activation after the residual sum (the strided layer's pre-activation)
    };
    std::vector<Stage> stages;
    // multiscale colour layer on this synthesis level's output (stride-1 reflect conv to the image channels), or null
    DevBuf color_wp;
    DevBuf color_bias;
    DevBuf color_wp16;  // f16x3 path: packed hi/lo weights of the colour layer
    DevBuf color_w4;    // colour layer from <= 128 to <= 4 channels: weights of color_small_kernel (both paths)
    int color_cout = 0;
    int act = 0;               // activation after the pre-convolution and after this layer (0 none, 1 LeakyReLU, 2 ReLU)
    DevBuf wp16;               // f16x3 path: packed hi/lo weights
    DevBuf gp16;               // f16x3 path: packed hi/lo gamma
    DevBuf wp_edge16;          // f16x3 path: packed weights of the first-conv / last-deconv kernel
    DevBuf wp_pmap16;          // f16x3 path, last synthesis layer (k = 3, cout <= 3): its weights as the product map
    bool f16_bad = false;      // a weight / gamma entry is not finite in f16: the model runs on the fp32 kernels
};

// Integer tables of the factorized entropy model + per-row encoder constants.
struct EntropyTables {
    int channels = 0, stride = 0;
    std::vector<int32_t> cdf, len, off;
    std::vector<float> medians;
    // encoder: per (row, value) exact-division constants (ryg_rans "Rans64EncSymbol" form)
    struct EncSym {
        uint64_t rcp_freq;   // fixed-point reciprocal
        uint32_t freq;
        uint32_t bias;
        uint32_t cmpl_freq;  // (1 << 16) - freq
        uint32_t rcp_shift;
    };
    std::vector<EncSym> enc;  // [channels * stride]
    static constexpr int kLutBits = 10;
    std::vector<uint16_t> lut;  // [channels << kLutBits]: first symbol of each cumulative-frequency bucket
    void build_tables();
};

// single chunks coded by the calling thread (cae_entropy.cpp); `headroom` bytes stay free in front of the stream
int rans_encode_chunk(const EntropyTables &T, const int32_t *symbols, int hw, size_t headroom, uint8_t **out,
                      size_t *out_len);
int rans_encode_chunk_pair(const EntropyTables &T, const int32_t *const *symbols, int hw, size_t headroom, uint8_t **out,
                           size_t *out_len);
int rans_decode_chunk(const EntropyTables &T, const uint8_t *buf, size_t len, int hw, int32_t *symbols);
int rans_decode_chunk_pair(const EntropyTables &T, const uint8_t *const *bufs, const size_t *lens, int hw,
                           int32_t *const *symbols);

// Device copy of EntropyTables for the device coder (cae_rans_device.hip): one buffer, byte offsets of its parts.
struct DevEntropy {
    DevBuf buf;
    uint64_t version = 0;  // Model::ent_version it was uploaded from
    size_t enc = 0, cdf = 0, lut = 0, len = 0, off = 0;
};

struct Model {
    int c_org = 0, c_net = 0, c_bn = 0, L = 0, ks = 3;
    std::vector<Layer> enc, dec;
    EntropyTables ent;
    uint64_t ent_version = 0;  // bumped by every cae_model_set_entropy
    DevEntropy ent_dev;
    int ensure_ent_device();   // (under `mu`)
    DevBuf medians_dev;
    bool medians_dirty = false;
    // factorized density network (cae_model_set_density): effective parameters, uniform width
    std::vector<float> density;
    int density_r = 0, density_k = 0, density_per_channel = 0;
    float density_bound = 0.f;
    int likelihood_plain = 1;  // cae_model_set_likelihood_form
    DevBuf density_dev;
    bool density_dirty = false;
    DevBuf bits_ws;  // [n * c_bn] doubles (cae_likelihood)
    DevBuf zero;
    DevBuf ws[4];    // converted input + three activation buffers
    std::mutex mu;
    // profiling: per track, per profiled call, the event pairs of every launched kernel
    int precision = 0;  // 0 = fp32 MFMA, 1 = f16x3 split MFMA
    bool profiling = false;
    std::vector<std::vector<std::pair<void *, void *>>> prof[2];
    // f16x3 range guard: ring of overflow words in pinned host memory (device-visible), one per call (ticket % kFlagSlots)
    static constexpr int kFlagSlots = 1024;
    int *flags = nullptr;      // host view
    int *flags_dev = nullptr;  // device view of the same words
    int64_t flag_seq = 0;
    int *next_flag(int64_t *ticket);  // takes a ticket, clears its word, remembers it as this thread's last ticket
    bool f16_usable() const;
    int ensure_ws(int which, size_t bytes);
    int ensure_device();
    // The workspaces are used in CALL order whatever stream a call names: a call on another stream than the one before
    // waits (on the device) for that one's work (order_stream, under `mu`).
    void *last_stream = nullptr;
    bool last_stream_set = false;
    void *order_event = nullptr;
    int order_stream(void *stream);
    ~Model();
};

}  // namespace cae
