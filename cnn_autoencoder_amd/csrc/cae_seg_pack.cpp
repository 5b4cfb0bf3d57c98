// The segmentation head's weight packer behind the C ABI (include/cae_hip.h): argument checks around pack_seg_f16
// (cae_pack.cpp).  Plain C++, no HIP include: the tests build it into a stand-alone sanitizer program.
#include <cstring>
#include <vector>

#include "cae_hip.h"
#include "cae_internal.hpp"
#include "cae_pack.hpp"

using namespace cae;

extern "C" {

size_t cae_seg_packed_halves(int cin_a, int cin_b, int cout, int ks, int up) {
    if (cin_a < 0 || cin_b < 0 || cin_a + cin_b < 1 || cout < 1 || (ks != 1 && ks != 3) || (up && (ks != 1 || cin_b))) return 0;
    const int m = seg_rows(cout, up != 0);
    return (size_t)seg_groups(m, ks) * seg_chunks(cin_a, cin_b) * ks * ks * seg_ct(m, ks) * 1024;
}

int cae_seg_pack(const float *w, int cin_a, int cin_b, int cout, int ks, int up, uint16_t *out, size_t capacity) {
    const size_t n = cae_seg_packed_halves(cin_a, cin_b, cout, ks, up);
    if (!w || !out) return fail(CAE_ERR_ARG, "NULL argument");
    if (!n) return fail(CAE_ERR_ARG, "cae_seg_pack: cin_a, cin_b >= 0 (sum >= 1), cout >= 1, ks 1 or 3; the transposed form has ks 1 and one source");
    if (capacity < n) return fail(CAE_ERR_ARG, "cae_seg_pack: %zu halves needed, room for %zu", n, capacity);
    const std::vector<_Float16> p = pack_seg_f16(w, cin_a, cin_b, cout, ks, up != 0);
    memcpy(out, p.data(), n * 2);
    return CAE_OK;
}

}  // extern "C"
