// Layout of every weight packer (the product's cae_pack.cpp) under AddressSanitizer / UBSan on the CPU: weights from a
// fixed integer recurrence, every packer over a fixed shape list, one "name hash" line (64-bit FNV-1a of the packed
// bytes) per case.  tests/test_pack_layout.py compares the lines with tests/golden/pack_layout.json.
#include "cae_pack.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace cae;

// values k / 2^20 with k a 24-bit integer: exact in fp32, and with low bits the hi half of the split format drops
static std::vector<float> fill(size_t n, uint64_t seed) {
    std::vector<float> v(n);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (auto &x : v) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x = (float)((int)(s >> 40) - (1 << 23)) * (1.0f / (1 << 20));
    }
    return v;
}

template <class T>
static void report(const char *name, const std::vector<T> &v, int a = -1, int b = -1, int c = -1, int d = -1, int e = -1) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    printf("%s", name);
    for (int x : {a, b, c, d, e})
        if (x >= 0) printf("/%d", x);
    printf(" %016llx\n", (unsigned long long)h);
}

int main() {
    const int couts[] = {27, 59, 96, 123, 187};  // channel tiles 1, 2, 4 (one empty), 4, 6
    const int cins[] = {3, 20, 96, 160, 192};    // not multiples of 8 / 16 / 32, and whole chunks
    for (int ks : {3, 5}) {
        for (int cout : couts)
            for (int cin : cins) {
                const auto w = fill((size_t)cin * cout * ks * ks, 1000u * cin + cout + ks);
                const int ct = round_ct(cout);
                for (int tr = 0; tr < 2; ++tr)
                    for (int flip = 0; flip < 2; ++flip) {
                        report("weights", pack_weights(w.data(), tr, cin, cout, ks, ct, flip), ks, cin, cout, tr, flip);
                        report("weights_f16", pack_weights_f16(w.data(), tr, cin, cout, ks, ct, flip), ks, cin, cout, tr, flip);
                    }
            }
        for (int cin : {1, 3, 4})
            for (int cout : couts) {
                const auto w = fill((size_t)cin * cout * ks * ks, 77u * cin + cout + ks);
                report("first", pack_first(w.data(), cin, cout, ks, round_ct(cout)), ks, cin, cout);
                report("first_f16", pack_first_f16(w.data(), cin, cout, ks, round_ct(cout)), ks, cin, cout);
            }
        for (int cout : {1, 3})
            for (int cin : cins) {
                const auto w = fill((size_t)cin * cout * ks * ks, 31u * cin + cout + ks);
                report("last", pack_last(w.data(), cin, cout, ks), ks, cin, cout);
                report("last_f16", pack_last_f16(w.data(), cin, cout, ks), ks, cin, cout);
            }
        for (int cout : {1, 3, 4})
            for (int cin : {20, 96, 128}) {
                const auto w = fill((size_t)cin * cout * ks * ks, 13u * cin + cout + ks);
                report("color4", pack_color4(w.data(), cin, cout, ks), ks, cin, cout);
            }
    }
    for (int cout : {1, 3})
        for (int cin : {96, 128}) {
            const auto w = fill((size_t)cin * cout * 9, 5u * cin + cout);
            report("pmap_f16", pack_pmap_f16(w.data(), cin, cout, round_ct(cin)), cin, cout);
        }
    for (int C : {48, 128, 192}) {
        const auto g = fill((size_t)C * C, C);
        report("gamma", pack_gamma(g.data(), C, round_ct(C)), C);
        report("gamma_f16", pack_gamma_f16(g.data(), C, round_ct(C)), C);
    }
    return 0;
}
