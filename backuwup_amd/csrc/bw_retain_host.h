// bw_retain_host.h -- the host arithmetic of retain (bw_retain.hip): the words of a root set, where a
// root's bit lies in an entry's mask, the check that a set holds no bit of a root that was not given, the
// drop predicate, and the order a forward sweep takes the levels of the edge list in.  Free of HIP so that
// a plain C++ test can include it (tests/cpp/retain_selftest.cpp).  Off the chunk -> hash -> dedup path.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "bw_impact_host.h"

namespace bw {

constexpr uint64_t RT_MAX_ROOTS = 4096;  // BW_RETAIN_MAX_ROOTS

// W: the u64 words of one root set; a set of no roots still has one
static inline uint64_t rt_words(uint64_t n_roots) { return n_roots ? (n_roots + 63) / 64 : 1; }

// masks are entry-major: root r's bit is bit rt_bit(r) of word rt_word(e, W, r)
static inline uint64_t rt_word(uint64_t e, uint64_t W, uint64_t r) { return e * W + r / 64; }
static inline uint64_t rt_bit(uint64_t r) { return 1ull << (r % 64); }

// the bits of word w (of W) that name a root below n_roots
static inline uint64_t rt_valid(uint64_t n_roots, uint64_t w) {
    if (64 * (w + 1) <= n_roots) return ~0ull;
    if (64 * w >= n_roots) return 0;
    return (1ull << (n_roots - 64 * w)) - 1;
}

// the first of n_rows sets of W words each that holds a bit at or past n_roots, or ~0
static inline uint64_t rt_foreign(const uint64_t* words, uint64_t n_rows, uint64_t W, uint64_t n_roots) {
    for (uint64_t w = n_roots / 64; w < W; w++) {  // the words before hold valid bits only
        const uint64_t bad = ~rt_valid(n_roots, w);
        for (uint64_t i = 0; i < n_rows; i++)
            if (words[i * W + w] & bad) return i;
    }
    return ~0ull;
}

// the drop predicate: an entry stays live when a root of its mask is not dropped
static inline bool rt_live(const uint64_t* mask, const uint64_t* drop, uint64_t W) {
    for (uint64_t w = 0; w < W; w++)
        if (mask[w] & ~drop[w]) return true;
    return false;
}

static inline bool rt_any(const uint64_t* mask, uint64_t W) {
    for (uint64_t w = 0; w < W; w++)
        if (mask[w]) return true;
    return false;
}

// one forward sweep's launches: the levels' ranges, earliest level first (the reverse of ImLevels::sweep,
// as the root sets go down the edges that impact's taint comes up), empty levels left out
static inline std::vector<std::pair<uint64_t, uint64_t>> rt_sweep(const ImLevels& L) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    for (uint64_t l = 0; l < L.n_levels(); l++)
        if (L.start[l + 1] > L.start[l]) out.push_back({L.start[l], L.start[l + 1]});
    return out;
}

}  // namespace bw
