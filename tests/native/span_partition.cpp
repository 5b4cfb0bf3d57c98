// The span partition of the plane histograms (csrc/cae_seg_span.hpp) walked on the host as the kernels walk it: every
// lane of every block of a plane takes its group turns, carrying its column by the per-turn step, then the first
// 2 (G - 1) lanes of the block take its singles.  For every case: every element of [0, lim) exactly once, none at or
// behind lim, the `on` flag of every visit equal to (p % row) < counted, every group at an aligned address, nothing from
// a block whose span is empty.  The same checks must call two deliberately wrong partitions wrong wherever they differ
// from the right one.  Prints "cases N ..." and exits 0, or the first failures and 1.
#include <cstdio>
#include <vector>

#include "cae_seg_span.hpp"

using cae::Span;

namespace {

enum Variant { kRight = 0, kNoHead = 1, kSinglesEverywhere = 2 };

struct Case {
    int G;
    size_t offset, row, plane_rows, rows, counted, bx, threads;
};

template <int G>
Span<G> span_for(const Case &k, size_t x, Variant variant) {
    // kNoHead: a head taken as 0 whatever the base's offset
    Span<G> s = cae::span_of<G>(variant == kNoHead ? 0 : k.offset, k.row, k.rows, k.counted, k.bx, x, k.threads);
    // kSinglesEverywhere: the singles given to every block instead of block 0
    if (variant == kSinglesEverywhere) s.singles = s.head + (s.lim - s.tail);
    return s;
}

// the walk of one plane -> what is wrong with it, or null
template <int G>
const char *walk(const Case &k, Variant variant) {
    constexpr size_t kSingleLanes = 2 * (size_t)(G - 1);
    const size_t plane = k.plane_rows * k.row;
    std::vector<int> seen(plane + G, 0);  // (a group that starts below lim ends below this)
    const char *wrong = nullptr;
    const auto visit = [&](size_t p, bool on, size_t lim) {
        if (p >= lim) wrong = "an element at or behind lim";
        if (p < seen.size()) seen[p] += 1;
        if (on != (p % k.row < k.counted)) wrong = "a wrong `on` flag";
    };
    size_t lim = 0;
    for (size_t x = 0; x < k.bx; ++x) {
        const Span<G> s = span_for<G>(k, x, variant);
        lim = s.lim;
        if (lim > plane) return "lim behind the plane";
        size_t visits = 0;
        for (size_t t = 0; t < k.threads; ++t) {
            size_t col = s.first_col(t);
            for (size_t g = s.g0 + t; g < s.g1; g += k.threads) {
                const size_t p = s.head + G * g;
                if ((k.offset + p) % G != 0) wrong = "a group off its alignment";
                if (p >= lim) return "a group at or behind lim";
                size_t c = col;
                for (int j = 0; j < G; ++j) {
                    visit(p + j, s.on(c), lim), ++visits;
                    if (++c == k.row) c = 0;
                }
                s.turn(col);
            }
        }
        if (s.singles > kSingleLanes) return "more singles than 2 (G - 1) lanes";
        for (size_t q = 0; q < kSingleLanes; ++q) {
            if (q < s.singles) {
                const size_t p = s.single(q);
                if (p >= lim) return "a single at or behind lim";
                visit(p, s.on(p % k.row), lim), ++visits;
            }
        }
        if (x != 0 && s.g0 == s.g1 && visits) wrong = "a visit from a block without a span";
    }
    for (size_t p = 0; p < lim; ++p)
        if (seen[p] != 1) return seen[p] ? "an element visited twice" : "an element left out";
    return wrong;
}

// whether the wrong partition differs from the right one in this case
template <int G>
bool differs(const Case &k, Variant variant) {
    const Span<G> s = span_for<G>(k, 0, kRight);
    if (variant == kNoHead) return k.offset == 1 && s.lim >= (size_t)G;  // a group of the wrong partition starts at 0
    return k.bx > 1 && s.singles > 0;
}

const char *walk(const Case &k, Variant v) { return k.G == 4 ? walk<4>(k, v) : walk<16>(k, v); }
bool differs(const Case &k, Variant v) { return k.G == 4 ? differs<4>(k, v) : differs<16>(k, v); }

}  // namespace

int main() {
    const size_t rows_of[] = {1, 2, 3, 5, 8, 17, 33}, planes[] = {1, 2, 3, 7}, blocks[] = {1, 2, 3, 7}, lanes[] = {1, 4, 64};
    long cases = 0, failures = 0, tried[3] = {0, 0, 0}, caught[3] = {0, 0, 0};
    for (int G : {4, 16})
        for (size_t offset = 0; offset < (size_t)G; ++offset)
            for (size_t row : rows_of)
                for (size_t plane_rows : planes)
                    for (size_t rows = 0; rows <= plane_rows; ++rows)
                        for (size_t counted = 0; counted <= row; ++counted)
                            for (size_t bx : blocks)
                                for (size_t threads : lanes) {
                                    const Case k = {G, offset, row, plane_rows, rows, counted, bx, threads};
                                    ++cases;
                                    const char *why = walk(k, kRight);
                                    if (why && ++failures <= 8)
                                        std::printf("wrong: %s: G=%d offset=%zu row=%zu plane_rows=%zu rows=%zu counted=%zu bx=%zu "
                                                    "threads=%zu\n", why, G, offset, row, plane_rows, rows, counted, bx, threads);
                                    for (Variant v : {kNoHead, kSinglesEverywhere}) {
                                        if (!differs(k, v)) continue;
                                        ++tried[v];
                                        if (walk(k, v)) ++caught[v];
                                    }
                                }
    for (Variant v : {kNoHead, kSinglesEverywhere}) {
        if (tried[v] == 0 || caught[v] != tried[v]) {
            std::printf("wrong partition %d passed the checks in %ld of %ld cases\n", (int)v, tried[v] - caught[v], tried[v]);
            ++failures;
        }
    }
    std::printf("cases %ld wrong_head %ld wrong_singles %ld\n", cases, caught[kNoHead], caught[kSinglesEverywhere]);
    return failures ? 1 : 0;
}
