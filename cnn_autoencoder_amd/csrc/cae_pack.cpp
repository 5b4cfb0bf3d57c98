// Weight packing of libcae_hip.so: the layouts the kernels read, written on the host (see cae_pack.hpp).
#include "cae_pack.hpp"

#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace cae {

int round_ct(int c) {
    const int t = (c + 31) / 32;
    if (t <= 1) return 1;
    if (t <= 2) return 2;
    if (t <= 4) return 4;
    if (t <= 6) return 6;
    return -1;
}

bool fits_f16(const float *v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(std::fabs(v[i]) <= 65504.0f)) return false;
    return true;
}

std::vector<float> pad_channels(const float *v, int c, int ct, float fill) {
    std::vector<float> out(ct * 32, fill);
    std::copy(v, v + c, out.begin());
    return out;
}

// ---- packing -----------------------------------------------------------------------------------
// weights -> [chunk][ky][kx][ct][lane][j]:  value W(cout = 32ct + (lane&31), cin = 8chunk + 4(lane>>5) + j, ky, kx)
std::vector<float> pack_weights(const float *w, bool transposed, int cin, int cout, int ks, int ct, bool flip) {
    const int chunks = (cin + 7) / 8;
    std::vector<float> out((size_t)chunks * ks * ks * ct * 256, 0.0f);
    size_t o = 0;
    for (int c = 0; c < chunks; ++c)
        for (int ky = 0; ky < ks; ++ky)
            for (int kx = 0; kx < ks; ++kx)
                for (int t = 0; t < ct; ++t)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j, ++o) {
                            const int co = 32 * t + (lane & 31);
                            const int ci = 8 * c + 4 * (lane >> 5) + j;
                            if (co < cout && ci < cin) {
                                // conv: (cout,cin,k,k); transposed conv: (cin,cout,k,k)
                                const int sy = flip ? ks - 1 - ky : ky, sx = flip ? ks - 1 - kx : kx;
                                const size_t idx = transposed ? (((size_t)ci * cout + co) * ks + sy) * ks + sx
                                                              : (((size_t)co * cin + ci) * ks + sy) * ks + sx;
                                out[o] = w[idx];
                            }
                        }
    return out;
}

// colour layer to <= 4 channels (color_small_kernel) -> [chunk][ky][kx][8 channels][4 outputs], zero padded
std::vector<float> pack_color4(const float *w, int cin, int cout, int ks) {
    const int chunks = (cin + 7) / 8;
    std::vector<float> out((size_t)chunks * ks * ks * 32, 0.0f);
    for (int ci = 0; ci < cin; ++ci)
        for (int ky = 0; ky < ks; ++ky)
            for (int kx = 0; kx < ks; ++kx)
                for (int co = 0; co < cout; ++co)
                    out[((((size_t)(ci >> 3) * ks + ky) * ks + kx) * 8 + (ci & 7)) * 4 + co] =
                        w[(((size_t)co * cin + ci) * ks + ky) * ks + kx];
    return out;
}

// gamma -> [jt][co][q][lane][jj]: value G(c = 32co + (lane&31), j = 32jt + row(4q+jj) + 4(lane>>5))
std::vector<float> pack_gamma(const float *g, int C, int ct) {
    std::vector<float> out((size_t)ct * ct * 4 * 256, 0.0f);
    size_t o = 0;
    for (int jt = 0; jt < ct; ++jt)
        for (int co = 0; co < ct; ++co)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int jj = 0; jj < 4; ++jj, ++o) {
                        const int s = 4 * q + jj;
                        const int c = 32 * co + (lane & 31);
                        const int j = 32 * jt + (s & 3) + 8 * (s >> 2) + 4 * (lane >> 5);
                        if (c < C && j < C) out[o] = g[(size_t)c * C + j];
                    }
    return out;
}

// first analysis layer (cin <= 4): [tap][ct][lane][2]: W(cout = 32ct + (lane&31), ch = 2j + (lane>>5), tap)
std::vector<float> pack_first(const float *w, int cin, int cout, int ks, int ct) {
    std::vector<float> out((size_t)ks * ks * ct * 128, 0.0f);
    size_t o = 0;
    for (int tap = 0; tap < ks * ks; ++tap)
        for (int t = 0; t < ct; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 2; ++j, ++o) {
                    const int co = 32 * t + (lane & 31), ch = 2 * j + (lane >> 5);
                    if (co < cout && ch < cin) out[o] = w[((size_t)co * cin + ch) * ks * ks + tap];
                }
    return out;
}

// neighbour offsets d = dlo .. dlo + nb - 1 of the last synthesis layer: output pixel (2y + py) reads input rows y + d
// through kernel rows ky = 2d + py + P
struct LastTaps {
    int P, dlo, nb;
    explicit LastTaps(int ks) : P(ks / 2), dlo(-((P + 1) / 2)), nb((ks - 1 - P) / 2 - dlo + 1) {}
};

// W[ci][c][ky][kx] of a transposed convolution (cin, cout, k, k), 0 outside the kernel / the real channels
static float last_weight(const float *w, int cin, int cout, int ks, int ci, int c, int ky, int kx) {
    if (c < cout && ci < cin && ky >= 0 && ky < ks && kx >= 0 && kx < ks) return w[(((size_t)ci * cout + c) * ks + ky) * ks + kx];
    return 0.0f;
}

// last synthesis layer (cout <= 4): [nd][ndx][q][lane][s]:
//   A(row = lane&15 = 4c + 2py + px, cin = 16q + 4(lane>>4) + s) = W[cin][c][2d+py+P][2dx+px+P]
std::vector<float> pack_last(const float *w, int cin, int cout, int ks) {
    const LastTaps t(ks);
    const int nq = (cin + 15) / 16;
    std::vector<float> out((size_t)t.nb * t.nb * nq * 256, 0.0f);
    size_t o = 0;
    for (int nd = 0; nd < t.nb; ++nd)
        for (int ndx = 0; ndx < t.nb; ++ndx)
            for (int q = 0; q < nq; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s2 = 0; s2 < 4; ++s2, ++o) {
                        const int row = lane & 15, c = row >> 2, py = (row >> 1) & 1, px = row & 1;
                        const int ci = 16 * q + 4 * (lane >> 4) + s2;
                        out[o] = last_weight(w, cin, cout, ks, ci, c, 2 * (t.dlo + nd) + py + t.P, 2 * (t.dlo + ndx) + px + t.P);
                    }
    return out;
}

// ---- f16x3 packing -------------------------------------------------------------------------------
// The one writer of the split format: `shape` is the record grid (row-major), a record is [hl][lane][8] halves, and
// value(r, lane, j) is the fp32 entry of record r (its index per dimension of `shape`); hi = f16(v), lo = f16(v - hi).
template <class F>
static std::vector<_Float16> pack_split(std::initializer_list<int> shape, F value) {
    std::vector<int> dims(shape), r(dims.size(), 0);
    size_t records = 1;
    for (int d : dims) records *= (size_t)d;
    std::vector<_Float16> out(records * 1024, (_Float16)0.0f);
    for (size_t rec = 0; rec < records; ++rec) {
        _Float16 *hi = out.data() + rec * 1024, *lo = hi + 512;
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const float v = value(r.data(), lane, j);
                hi[lane * 8 + j] = (_Float16)v;
                lo[lane * 8 + j] = (_Float16)(v - (float)hi[lane * 8 + j]);
            }
        for (size_t d = dims.size(); d-- > 0 && ++r[d] == dims[d];) r[d] = 0;  // next record index
    }
    return out;
}

// weights -> [q][ky][kx][ct][hl][lane][8]: W(cout = 32ct + (lane&31), cin = 16q + 8(lane>>5) + j, ky, kx)
std::vector<_Float16> pack_weights_f16(const float *w, bool transposed, int cin, int cout, int ks, int ct, bool flip) {
    return pack_split({(cin + 15) / 16, ks, ks, ct}, [=](const int *r, int lane, int j) {
        const int q = r[0], ky = r[1], kx = r[2], t = r[3];
        const int co = 32 * t + (lane & 31);
        const int ci = 16 * q + 8 * (lane >> 5) + j;
        if (co >= cout || ci >= cin) return 0.0f;
        const int sy = flip ? ks - 1 - ky : ky, sx = flip ? ks - 1 - kx : kx;
        return transposed ? w[(((size_t)ci * cout + co) * ks + sy) * ks + sx]
                          : w[(((size_t)co * cin + ci) * ks + sy) * ks + sx];
    });
}

// gamma -> [jt][co][s][hl][lane][8]: G(c = 32co + (lane&31), j = 32jt + row(8s+e) + 4(lane>>5))
std::vector<_Float16> pack_gamma_f16(const float *g, int C, int ct) {
    return pack_split({ct, ct, 2}, [=](const int *r, int lane, int e) {
        const int jt = r[0], co = r[1], row = 8 * r[2] + e;
        const int c = 32 * co + (lane & 31);
        const int j = 32 * jt + (row & 3) + 8 * (row >> 2) + 4 * (lane >> 5);
        return (c < C && j < C) ? g[(size_t)c * C + j] : 0.0f;
    });
}

// first layer f16x3: [s][ct][hl][lane][8]: W(cout = 32ct + (lane&31), tap = 4s + 2(lane>>5) + (j>>2), ch = j&3)
std::vector<_Float16> pack_first_f16(const float *w, int cin, int cout, int ks, int ct) {
    return pack_split({(ks * ks + 3) / 4, ct}, [=](const int *r, int lane, int j) {
        const int co = 32 * r[1] + (lane & 31), tap = 4 * r[0] + 2 * (lane >> 5) + (j >> 2), ch = j & 3;
        return (co < cout && ch < cin && tap < ks * ks) ? w[((size_t)co * cin + ch) * ks * ks + tap] : 0.0f;
    });
}

// last layer f16x3: [nd][ndx][q][hl][lane][8]: A(row = lane&15 = 4c + 2py + px, cin = 32q + 8(lane>>4) + j)
std::vector<_Float16> pack_last_f16(const float *w, int cin, int cout, int ks) {
    const LastTaps t(ks);
    return pack_split({t.nb, t.nb, (cin + 31) / 32}, [=](const int *r, int lane, int j) {
        const int row = lane & 15, c = row >> 2, py = (row >> 1) & 1, px = row & 1;
        const int ci = 32 * r[2] + 8 * (lane >> 4) + j;
        return last_weight(w, cin, cout, ks, ci, c, 2 * (t.dlo + r[0]) + py + t.P, 2 * (t.dlo + r[1]) + px + t.P);
    });
}

// last layer as a product map (cae_kernels_f16.hpp, pmap): [jt][s][hl][lane][8]:
//   A(row = lane&31 = 3 tap + c, k = 32jt + row(8s+e) + 4(lane>>5)) = W[cin = k][c][ky][kx], tap = 3 ky + kx  (k = 3)
std::vector<_Float16> pack_pmap_f16(const float *w, int cin, int cout, int njt) {
    // njt = channel tiles of the PRODUCING layer's accumulators (round_ct(cin): 96 channels live in 4 tiles), zero padded
    return pack_split({njt, 2}, [=](const int *r, int lane, int e) {
        // map row (lane & 31) = slot of the record as pmap_gather_kernel reads it (cae_kernels_f16.hpp):
        // [taps 4, 5, 7, 8 | taps 3, 6, pad 2 | taps 1, 2, pad 2 | tap 0, pad 1] x 3 channels
        static const int slot_tap[32] = {4, 4, 4, 5, 5, 5, 7, 7, 7, 8, 8, 8, 3, 3, 3, 6, 6, 6, -1, -1,
                                         1, 1, 1, 2, 2, 2, -1, -1, 0, 0, 0, -1};
        static const int slot_c[32] = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 0,
                                       0, 1, 2, 0, 1, 2, 0, 0, 0, 1, 2, 0};
        const int row = 8 * r[1] + e, slot = lane & 31, tap = slot_tap[slot], c = slot_c[slot];
        const int j = 32 * r[0] + (row & 3) + 8 * (row >> 2) + 4 * (lane >> 5);
        return (tap >= 0 && c < cout && j < cin) ? w[((size_t)j * cout + c) * 9 + tap] : 0.0f;
    });
}

// ---- segmentation head (cae_kernels_seg.hpp) --------------------------------------------------------------
// channel tiles per block of seg_conv_f16_kernel<ks, ct> for m output rows, and the groups of such tiles over the grid
int seg_ct(int m, int ks) {
    if (m <= 32) return 1;
    if (m <= 64 || ks == 3) return 2;
    return 4;
}
int seg_groups(int m, int ks) { return (m + 32 * seg_ct(m, ks) - 1) / (32 * seg_ct(m, ks)); }
int seg_rows(int cout, bool up) { return up ? 4 * ((cout + 7) / 8 * 8) : cout; }
int seg_chunks(int cin_a, int cin_b) { return ((cin_a + 7) / 8 + (cin_b + 7) / 8 + 1) / 2; }

// [group][q][ky][kx][ct][hl][lane][8]: W(row = 32 (group CT + ct) + (lane&31), k = 16q + 8(lane>>5) + j, ky, kx).
// k runs over the concatenated PLANE grid of the two sources: the ceil(cin_a / 8) planes of source A, then source B's;
// the padding channels of either source's last plane (and of an odd last plane pair) are zero rows.
//   conv (up = false): w is (cout, cin_a + cin_b, ks, ks), row = cout index.
//   2x2 stride-2 transposed conv (up = true, ks = 1): w is (cin_a, cout, 2, 2); row = (2 dy + dx) CP + co with
//   CP = cout rounded up to whole planes: four pointwise matrices, one per output parity.
std::vector<_Float16> pack_seg_f16(const float *w, int cin_a, int cin_b, int cout, int ks, bool up) {
    const int m = seg_rows(cout, up), ct = seg_ct(m, ks), groups = seg_groups(m, ks);
    const int pa = (cin_a + 7) / 8, cp = (cout + 7) / 8 * 8, cin = cin_a + cin_b;
    return pack_split({groups, seg_chunks(cin_a, cin_b), ks, ks, ct}, [=](const int *r, int lane, int j) {
        const int row = 32 * (r[0] * ct + r[4]) + (lane & 31), k = 16 * r[1] + 8 * (lane >> 5) + j;
        int ci;
        if (k < 8 * pa) {
            if (k >= cin_a) return 0.0f;
            ci = k;
        } else {
            if (k - 8 * pa >= cin_b) return 0.0f;
            ci = cin_a + k - 8 * pa;
        }
        if (row >= m) return 0.0f;
        if (up) {
            const int par = row / cp, co = row % cp;
            return co < cout ? w[((size_t)ci * cout + co) * 4 + par] : 0.0f;
        }
        return w[(((size_t)row * cin + ci) * ks + r[2]) * ks + r[3]];
    });
}

}  // namespace cae
