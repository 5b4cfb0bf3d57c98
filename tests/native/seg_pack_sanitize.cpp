// The segmentation head's host packers (cae_pack.cpp, cae_seg_pack.cpp, unchanged) and their argument checks under AddressSanitizer +
// UBSan: ragged channel counts on both sides of a concat boundary, every kernel-size / transposed form, group counts
// from one to many, outputs that are too small, arguments that must be refused.  Stand-alone: its own main, no GPU.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_pack.hpp"

namespace cae {
static std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
void dev_free(void *) {}
}  // namespace cae

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// value of (row, k, tap) read back from the fragment order
static double at(const std::vector<uint16_t> &p, int chunks, int ks, int ct, int row, int k, int tap) {
    const int g = row / (32 * ct), t = row / 32 % ct, lane = (row & 31) + 32 * ((k >> 3) & 1), q = k / 16, j = k & 7;
    const size_t rec = (((size_t)g * chunks + q) * ks * ks + tap) * ct + t;
    _Float16 hi, lo;
    memcpy(&hi, &p[rec * 1024 + lane * 8 + j], 2);
    memcpy(&lo, &p[rec * 1024 + 512 + lane * 8 + j], 2);
    return (double)hi + (double)lo;
}

int main() {
    unsigned seed = 1;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)((seed >> 8) & 0xffff) / 65536.0f - 0.5f; };
    int cases = 0;
    for (int ks : {1, 3})
        for (int up = 0; up < 2; ++up)
            for (int ca : {0, 1, 5, 8, 20, 33})
                for (int cb : {0, 3, 8, 20})
                    for (int cout : {1, 5, 8, 31, 33, 70, 150}) {
                        const size_t n = cae_seg_packed_halves(ca, cb, cout, ks, up);
                        if (ca + cb == 0 || (up && (ks != 1 || cb))) {
                            CHECK(n == 0);
                            continue;
                        }
                        const int cin = ca + cb, taps = up ? 4 : ks * ks;
                        std::vector<float> w((size_t)cin * cout * taps);
                        for (float &v : w) v = rnd();
                        std::vector<uint16_t> out(n);
                        CHECK(cae_seg_pack(w.data(), ca, cb, cout, ks, up, out.data(), n) == CAE_OK);
                        CHECK(cae_seg_pack(w.data(), ca, cb, cout, ks, up, out.data(), n - 1) == CAE_ERR_ARG);
                        const int m = cae::seg_rows(cout, up != 0), ct = cae::seg_ct(m, ks), chunks = cae::seg_chunks(ca, cb);
                        CHECK(n == (size_t)cae::seg_groups(m, ks) * chunks * ks * ks * ct * 1024);
                        const int pa = (ca + 7) / 8, cp = (cout + 7) / 8 * 8;
                        for (int row = 0; row < cae::seg_groups(m, ks) * ct * 32; ++row)
                            for (int k = 0; k < chunks * 16; ++k)
                                for (int tap = 0; tap < ks * ks; ++tap) {
                                    int ci = -1;
                                    if (k < 8 * pa) ci = k < ca ? k : -1;
                                    else if (k - 8 * pa < cb) ci = ca + k - 8 * pa;
                                    double want = 0.0;
                                    if (ci >= 0 && row < m) {
                                        if (up) {
                                            const int par = row / cp, co = row % cp;
                                            if (co < cout) want = w[((size_t)ci * cout + co) * 4 + par];
                                        } else {
                                            want = w[((size_t)row * cin + ci) * ks * ks + tap];
                                        }
                                    }
                                    const double got = at(out, chunks, ks, ct, row, k, tap);
                                    const double tol = want == 0.0 ? 0.0 : 1.0 / (1 << 22) * (want < 0 ? -want : want) + 1.0 / (1 << 25);
                                    CHECK((got - want < 0 ? want - got : got - want) <= tol);
                                }
                        ++cases;
                    }
    // refused arguments
    std::vector<float> w(64, 1.0f);
    std::vector<uint16_t> out(4096);
    CHECK(cae_seg_pack(nullptr, 4, 0, 4, 1, 0, out.data(), out.size()) == CAE_ERR_ARG);
    CHECK(cae_seg_pack(w.data(), 4, 0, 4, 1, 0, nullptr, out.size()) == CAE_ERR_ARG);
    CHECK(cae_seg_pack(w.data(), -1, 4, 4, 1, 0, out.data(), out.size()) == CAE_ERR_ARG);
    CHECK(cae_seg_pack(w.data(), 4, 0, 0, 1, 0, out.data(), out.size()) == CAE_ERR_ARG);
    CHECK(cae_seg_pack(w.data(), 4, 0, 4, 2, 0, out.data(), out.size()) == CAE_ERR_ARG);
    CHECK(cae_seg_pack(w.data(), 4, 0, 4, 3, 1, out.data(), out.size()) == CAE_ERR_ARG);
    CHECK(!cae::g_err.empty());
    const float big[2] = {65504.0f, 65505.0f};
    CHECK(cae::fits_f16(big, 1) && !cae::fits_f16(big, 2));
    printf("seg_pack_sanitize: ok (%d shapes)\n", cases);
    return 0;
}
