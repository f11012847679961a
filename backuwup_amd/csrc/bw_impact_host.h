// bw_impact_host.h -- the host arithmetic of impact (bw_impact.hip): the check that a taint vector holds
// only the two public bits, the room a sub-batch's edges need, and the layout of the edge list by the
// level that appended them, with the order a sweep takes them in.  Free of HIP so that a plain C++ test
// can include it (tests/test_impact_host.py).  Off the chunk -> hash -> dedup path.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

namespace bw {

constexpr uint32_t IM_SELF = 1, IM_BELOW = 2;  // BW_IMPACT_SELF, BW_IMPACT_BELOW
constexpr uint64_t IM_MAX_ENTRIES = 1ull << 31;  // an edge names an entry in 31 bits
constexpr uint32_t IM_EDGE_SELF_ONLY = 0x80000000u;  // on an edge's child: a File row, which looks at SELF only

// the first entry whose taint byte holds another bit than the two, or ~0
static inline uint64_t im_taint_check(const uint8_t* taint, uint64_t n) {
    for (uint64_t e = 0; e < n; e++)
        if (taint[e] & ~(IM_SELF | IM_BELOW)) return e;
    return ~0ull;
}

// No more edges than this can a sub-batch of m decoded blobs append: a blob the chain refused (cst)
// appends none; a decoded one of len bytes holds its children rows and its next_sibling, 32 bytes each,
// so it names at most len / 32 hashes, whatever the parser will say of it.
static inline uint64_t im_edge_bound(const uint8_t* cst, const uint64_t* len, uint64_t m) {
    uint64_t n = 0;
    for (uint64_t k = 0; k < m; k++)
        if (!cst[k]) n += len[k] / 32;
    return n;
}

// The edge list by level: level l appended the edges [start[l], start[l + 1]).
struct ImLevels {
    std::vector<uint64_t> start = {0};
    // the walk finished a level with n_edges in the list; false when the count went backwards
    bool close(uint64_t n_edges) {
        if (n_edges < start.back()) return false;
        start.push_back(n_edges);
        return true;
    }
    uint64_t n_levels() const { return start.size() - 1; }
    uint64_t n_edges() const { return start.back(); }
    // one sweep's launches: the levels' ranges, latest level first, empty levels left out
    std::vector<std::pair<uint64_t, uint64_t>> sweep() const {
        std::vector<std::pair<uint64_t, uint64_t>> out;
        for (uint64_t l = n_levels(); l-- > 0;)
            if (start[l + 1] > start[l]) out.push_back({start[l], start[l + 1]});
        return out;
    }
};

}  // namespace bw
