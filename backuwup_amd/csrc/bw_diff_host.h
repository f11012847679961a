// bw_diff_host.h -- the diff walk's host-only sizing rules (bw_diff.hip), free of HIP so that a plain
// C++ test can include them (tests/test_diff_walk.py).  Off the chunk -> hash -> dedup path.
#pragma once
#include <stdint.h>

namespace bw {

// Rows, and nodes, of one level: the tables hold u32 indices and twice as many slots as keys.  A level
// beyond this ends the walk (BW_ENOMEM).
constexpr uint64_t DF_MAX_ROWS = 1ull << 30;

// The capacity of a table of n keys: a power of two of at least 2 n, and of at least 64.  For
// n <= DF_MAX_ROWS it fits 32 bits; the count is kept in 64 bits and ends at 2^31 whatever n is.
static inline uint32_t df_table_cap(uint64_t n) {
    uint64_t cap = 64;
    while (cap < 2 * n && cap < (1ull << 31)) cap <<= 1;
    return (uint32_t)cap;
}

}  // namespace bw
