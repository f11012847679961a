// bw_find.h -- private declarations of find (bw_find.hip): the items of the walk, its device state as the
// kernels take it, and the session's buffers.  References, the take table and the fetch's state are
// bw_walk.h's, shared with the diff walk, the parent match and impact's report walk; the pattern
// language and its per-byte rule are bw_find_host.h's.  Off the chunk -> hash -> dedup path
// (backuwup_amd/build.py OFF_PATH), like bw_impact.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/backuwup_gpu.h"
#include "bw_walk.h"
#include "bw_find_host.h"

namespace bw {

constexpr uint64_t FD_MAX_ROWS = 1ull << 30;  // the walk indexes a level in 32 bits
constexpr uint64_t FD_NONE = ~0ull;
constexpr uint32_t FD_MATCH_BLOCKS = 512;  // k_fd_match's grid at most: two workgroups a CU at 32 patterns

// the session's buffers (bw_restore::fd)
enum {
    FD_B_ITEMS0, FD_B_ITEMS1, FD_B_REFS0, FD_B_REFS1, FD_B_ST0, FD_B_ST1, FD_B_LVL, FD_B_LVL2, FD_B_REC, FD_B_PAT,
    FD_B_CODE, FD_B_XMAP, FD_B_XREFS, FD_B_TAB, FD_B_CHUNKS,
    FD_B_COUNT
};
static_assert(FD_B_COUNT <= sizeof(bw_restore::fd) / sizeof(DevBuf), "bw_restore::fd holds every buffer");

// an item's state
constexpr uint32_t FD_OK = 1;      // its first piece was read and parsed
constexpr uint32_t FD_CYCLIC = 2;  // its hash is one of its ancestors'
constexpr uint32_t FD_TRUNC = 4;   // a later piece of its chain is lost
constexpr uint32_t FD_ALIVE = 8;   // some pattern's carried state is not empty

// what k_fd_decide tells the host of an item
constexpr uint8_t FD_X_NONE = 0, FD_X_DIR = 1, FD_X_CHUNKS = 2, FD_X_PRUNED = 3;

// One item of a level.
struct FdItem {
    uint8_t hash[32];
    uint64_t parent;  // the parent item's record, ~0 for a root
    uint32_t root, state;
    uint32_t kind, tflags;
    uint64_t size, mtime, ctime;
    uint64_t name_off, name_len;  // in the walk's name arena
    uint32_t inherit;   // the parent's pattern bits (BW_FIND_SUBTREE)
    uint32_t patterns;  // k_fd_match: the patterns its path matches; k_fd_decide: the inherited ones too
    uint32_t flags, pad;  // k_fd_decide: BW_FIND_HIT, BW_FIND_PRUNED
};

struct FdQuery {
    uint32_t n_patterns, kinds, flags, pad;
    uint64_t size_min, size_max, mtime_min, mtime_max;
};

// The walk's device state.
struct FdWalk {
    WkFetch f;  // the shared fetch; f.names holds every name so far
    FdItem* items;
    bw_find_record* recs;  // every record so far; item i of the level owns record rec0 + i
    uint64_t n_items, level, rec0;
    uint64_t rec0_prev;  // the first record of the level above: a child's parent item is parent - rec0_prev
    const uint64_t* masks;  // [byte][pattern]: the compiled byte masks
    const FdPat* pats;
    const uint64_t* st_prev;  // [item of the level above][pattern]: the carried states
    uint64_t* st_cur;
    FdQuery q;
};

}  // namespace bw
