// Host-side packing of weights into the layouts the kernels read (cae_pack.cpp; plain C++, no HIP include).
#pragma once
#include <cstddef>
#include <vector>

namespace cae {

// 32-channel tiles the kernels are built for (1, 2, 4, 6), or -1 above 192 channels
int round_ct(int c);
// every entry representable in the split format (finite, |v| <= 65504)?
bool fits_f16(const float *v, size_t n);
// per-channel vector padded to ct*32 entries with `fill` (bias: 0, beta: 1)
std::vector<float> pad_channels(const float *v, int c, int ct, float fill);

std::vector<float> pack_weights(const float *w, bool transposed, int cin, int cout, int ks, int ct, bool flip = false);
std::vector<float> pack_color4(const float *w, int cin, int cout, int ks);
std::vector<float> pack_gamma(const float *g, int C, int ct);
std::vector<float> pack_first(const float *w, int cin, int cout, int ks, int ct);
std::vector<float> pack_last(const float *w, int cin, int cout, int ks);

// f16x3: every value as a (hi, lo) pair of halves, records of [hl][lane][8]
std::vector<_Float16> pack_weights_f16(const float *w, bool transposed, int cin, int cout, int ks, int ct,
                                       bool flip = false);
std::vector<_Float16> pack_gamma_f16(const float *g, int C, int ct);
std::vector<_Float16> pack_first_f16(const float *w, int cin, int cout, int ks, int ct);
std::vector<_Float16> pack_last_f16(const float *w, int cin, int cout, int ks);
std::vector<_Float16> pack_pmap_f16(const float *w, int cin, int cout, int njt);

// segmentation head: launch shape of a layer with m output rows, and its packed f16x3 weights (cae_pack.cpp)
int seg_ct(int m, int ks);
int seg_groups(int m, int ks);
int seg_rows(int cout, bool up);
int seg_chunks(int cin_a, int cin_b);
std::vector<_Float16> pack_seg_f16(const float *w, int cin_a, int cin_b, int cout, int ks, bool up);

}  // namespace cae
