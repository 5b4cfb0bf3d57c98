// The span partition of the plane histograms (roc_hist_kernel and score_hist_kernel, cae_seg_hist.hip;
// tile_byte_hist_kernel, cae_tiles.hip), once: which elements of a plane a block takes G at a time behind aligned
// addresses, which are left to single lanes, and where in its row a lane stands.  Plain arithmetic on sizes, so that a
// host program can walk it too (tests/native/span_partition.cpp).
//
// A plane is `row` elements wide.  Its first `rows` rows are counted, and of each row the first `counted` elements: the
// elements [0, lim) are visited, those at a column >= counted are loaded and left out (`ragged`).  [head, tail) are
// `groups` whole groups of G elements, the first of each at an address that is a multiple of G elements; block x of the
// plane's bx takes the contiguous groups [g0, g1), lane t of it the groups g0 + t, g0 + t + threads, ...  The
// head + (lim - tail) <= 2 (G - 1) others are the singles: one per lane of block 0.
#pragma once
#include <cstddef>

#if defined(__HIP__)
#define CAE_SPAN_FN __host__ __device__ inline
#else
#define CAE_SPAN_FN inline
#endif

namespace cae {

template <int G>
struct Span {
    static_assert(G > 0 && (G & (G - 1)) == 0, "a group is a power of two of elements");
    size_t row, counted;  // elements of a row, and those of them that count
    size_t lim, head, groups, g0, g1, tail, singles;
    size_t dcol;          // what a turn of `threads` groups adds to a lane's column, below row
    bool ragged;

    // the column of the first element of lane t's first group; 0 where no column is looked at
    CAE_SPAN_FN size_t first_col(size_t t) const { return ragged && g0 + t < g1 ? (head + G * (g0 + t)) % row : 0; }
    // ... and of the group one turn on
    CAE_SPAN_FN void turn(size_t &col) const {
        col += dcol;
        if (col >= row) col -= row;
    }
    // whether the element at this column counts
    CAE_SPAN_FN bool on(size_t col) const { return !ragged || col < counted; }
    // single q of 0 .. singles -> its element, below lim
    CAE_SPAN_FN size_t single(size_t q) const { return q < head ? q : tail + (q - head); }
};

// elements in front of the first address at or behind p that is a multiple of G elements (p aligned to its elements)
template <int G, typename T>
CAE_SPAN_FN size_t span_offset(const T *p) {
    return (size_t)((reinterpret_cast<size_t>(p) / sizeof(T)) & (size_t)(G - 1));
}
template <int G>
CAE_SPAN_FN size_t span_head(size_t offset) {
    return (0 - offset) & (size_t)(G - 1);
}

// offset: span_offset of the plane's base; rows, counted: as extent_of gives them, inside the plane
template <int G>
CAE_SPAN_FN Span<G> span_of(size_t offset, size_t row, size_t rows, size_t counted, size_t bx, size_t x, size_t threads) {
    Span<G> s;
    s.row = row, s.counted = counted;
    s.lim = counted > 0 ? rows * row : 0;  // whole rows beyond `rows` are never loaded
    s.ragged = counted < row;              // columns beyond `counted` are loaded and left out
    s.head = s.lim < span_head<G>(offset) ? s.lim : span_head<G>(offset);
    s.groups = (s.lim - s.head) / G;
    const size_t per_block = (s.groups + bx - 1) / bx;
    s.g0 = s.groups < x * per_block ? s.groups : x * per_block;
    s.g1 = s.groups < s.g0 + per_block ? s.groups : s.g0 + per_block;
    s.tail = s.head + G * s.groups;
    s.singles = x == 0 ? s.head + (s.lim - s.tail) : 0;  // block 0 takes them
    s.dcol = (G * threads) % row;
    return s;
}

}  // namespace cae
